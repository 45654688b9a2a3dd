"""Fixtures of the CAWN tests, produced by the REFERENCE itself: imports it from $DYGLIB_REFERENCE at run time (nothing of it is copied), loads
the seeded parameters of tests/cawn_cases.py with strict=True, runs the eval-mode forward on the CPU and writes

    tests/golden/cawn_<case>.npz  on ONE sampler (a random strategy's RandomState carries over) the embeddings of the (src, dst) call and
                                  then of the (src, neg_dst) call, the state_dict key list, and, from a call on the first TAP_ROWS pairs of
                                  (src, dst) after the sampler is reset: the walks' node ids, their appearance counts (from
                                  position_encoder.nodes_appearances), and the outputs of feature_encoder, position_encoder,
                                  projection_layers[0] and transformer_encoder (forward hooks), index 0 / 1 = source / destination side

Only outputs are stored; the tests rebuild the inputs from the recipes.

    DYGLIB_REFERENCE=<checkout of the reference> python tools/make_golden_cawn.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = os.environ.get("DYGLIB_REFERENCE")
if not REF:
    sys.exit("set DYGLIB_REFERENCE to a checkout of the reference (DyGLib)")
sys.path.insert(0, REF)

from tests import cawn_cases as cc  # noqa: E402
from tests import golden_cases as gc  # noqa: E402


def ref_model(c):
    from models.CAWN import CAWN
    from utils.DataLoader import Data
    from utils.utils import get_neighbor_sampler
    d, cfg = c["data"], c["cawn_cfg"]
    sampler = get_neighbor_sampler(Data(d.src_node_ids, d.dst_node_ids, d.node_interact_times, d.edge_ids, d.labels), cfg["strategy"],
                                   time_scaling_factor=cfg["scale"], seed=cfg["sampler_seed"])
    m = CAWN(c["node_feat"], c["edge_feat"], sampler, cc.TIME_FEAT_DIM, cfg["P"], walk_length=cfg["W"], num_walk_heads=cfg["heads"], dropout=0.1)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["cawn_params"].items()}, strict=True)
    return m.eval(), sampler


def make_case(name: str):
    c = cc.build_cawn_case(name)
    cfg = c["cawn_cfg"]
    k, W = cfg["k"], cfg["W"]
    M = k ** W
    m, sampler = ref_model(c)
    out = {"state_dict_keys": np.array(list(m.state_dict().keys()))}
    with torch.no_grad():
        m.set_neighbor_sampler(sampler)
        s, d = m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=k)
        sn, nd = m.compute_src_dst_node_temporal_embeddings(c["src"], c["neg_dst"], c["times"], num_neighbors=k)
        out["src_emb"], out["dst_emb"], out["src_neg_emb"], out["neg_dst_emb"] = s.numpy(), d.numpy(), sn.numpy(), nd.numpy()
        # every module below is called twice per forward: source side, then destination side
        we = m.walk_encoder
        mods = dict(feature_out=we.feature_encoder, position_out=we.position_encoder, attn_in=we.projection_layers[0], attn_out=we.transformer_encoder)
        calls = {key: [] for key in mods}
        hooks = [mod.register_forward_hook(lambda _m, _a, o, key=key: calls[key].append(o.numpy().copy())) for key, mod in mods.items()]
        ids = []
        hooks.append(m.position_encoder.register_forward_hook(lambda _m, _a, kw, _o: ids.append(kw["nodes_neighbor_ids"].copy()), with_kwargs=True))
        r = min(cc.TAP_ROWS, len(c["src"]))
        m.set_neighbor_sampler(sampler)                                  # resets a random sampler's state
        m.compute_src_dst_node_temporal_embeddings(c["src"][:r], c["dst"][:r], c["times"][:r], num_neighbors=k)
        for h in hooks:
            h.remove()
    assert all(len(v) == 2 for v in calls.values()) and len(ids) == 2
    for key, v in calls.items():
        out["tap_" + key] = np.stack([x.reshape(r, M, -1) for x in v], axis=1)
    out["tap_walk_ids"] = np.stack(ids, axis=1).astype(np.int64)
    table = m.position_encoder.nodes_appearances
    out["tap_counts"] = np.array([[[[table[f"{i}-{v}"] for v in walk] for walk in side] for side in pair] for i, pair in enumerate(out["tap_walk_ids"])],
                                 dtype=np.float32)
    assert out["tap_counts"].shape == (r, 2, M, W + 1, 2, W + 1)
    assert np.isfinite(out["src_emb"]).all() and np.isfinite(out["src_neg_emb"]).all()
    lens = (out["tap_walk_ids"] != 0).sum(-1)
    print(f"{name}: max |emb| {np.abs(out['src_emb']).max():.3g}, max |src_pos - src_neg| {np.abs(out['src_emb'] - out['src_neg_emb']).max():.3g}, "
          f"tap walk lengths {np.bincount(lens.ravel(), minlength=W + 2).tolist()}, both count rows non-zero at "
          f"{int(((out['tap_counts'][..., 0, :].sum(-1) > 0) & (out['tap_counts'][..., 1, :].sum(-1) > 0)).sum())} positions, "
          f"empty histories src {int((c['hist_src'] == 0).sum())} dst {int((c['hist_dst'] == 0).sum())}, one-sided pair {c['one_sided']}")
    path = os.path.join(gc.GOLDEN_DIR, f"cawn_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    for name in (sys.argv[1:] or cc.CASES):
        make_case(name)
