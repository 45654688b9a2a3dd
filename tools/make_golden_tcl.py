"""Fixtures of the TCL tests, produced by the REFERENCE itself: imports it from $DYGLIB_REFERENCE at run time (nothing of it is copied), loads
the seeded parameters of tests/tcl_cases.py with strict=True, runs the eval-mode forward on the CPU and writes

    tests/golden/tcl_<case>.npz   on ONE sampler (a random strategy's RandomState carries over) the embeddings of the (src, dst) call and
                                  then of the (src, neg_dst) call, the state_dict key list, and, from a call on the first TAP_ROWS pairs of
                                  (src, dst) after the sampler is reset, the encoder input and every layer's two outputs (captured with
                                  forward hooks on the transformer blocks) with the sequences' node ids (0 = a padded position)
    tests/golden/eval_tcl.npz     per-batch loss / AP / AUC of the reference's evaluate_model_link_prediction("TCL", ...) and its negative
                                  draws

Only outputs are stored; the tests rebuild the inputs from the recipes.

    python tools/make_golden_tcl.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = os.environ.get("DYGLIB_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

from tests import golden_cases as gc  # noqa: E402
from tests import tcl_cases as tc  # noqa: E402


def ref_model(c):
    from models.TCL import TCL
    from utils.DataLoader import Data
    from utils.utils import get_neighbor_sampler
    d, cfg = c["data"], c["tcl_cfg"]
    sampler = get_neighbor_sampler(Data(d.src_node_ids, d.dst_node_ids, d.node_interact_times, d.edge_ids, d.labels), cfg["strategy"],
                                   seed=cfg["sampler_seed"])
    m = TCL(c["node_feat"], c["edge_feat"], sampler, tc.TIME_FEAT_DIM, num_layers=cfg["layers"], num_heads=cfg["heads"], num_depths=cfg["K"] + 1,
            dropout=0.1)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["tcl_params"].items()}, strict=True)
    return m.eval(), sampler


def make_case(name: str):
    c = tc.build_tcl_case(name)
    cfg = c["tcl_cfg"]
    K, layers = cfg["K"], cfg["layers"]
    m, sampler = ref_model(c)
    out = {"state_dict_keys": np.array(list(m.state_dict().keys()))}
    with torch.no_grad():
        m.set_neighbor_sampler(sampler)
        s, d = m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=K)
        sn, nd = m.compute_src_dst_node_temporal_embeddings(c["src"], c["neg_dst"], c["times"], num_neighbors=K)
        out["src_emb"], out["dst_emb"], out["src_neg_emb"], out["neg_dst_emb"] = s.numpy(), d.numpy(), sn.numpy(), nd.numpy()
        # every block is called four times per forward: self a, self b, cross a, cross b (keyword arguments only)
        calls = [[] for _ in range(layers)]
        hooks = [t.register_forward_hook(lambda mod, a, kw, o, l=l: calls[l].append((kw["inputs_query"].numpy().copy(), kw["neighbor_masks"].copy(),
                                                                                      o.numpy().copy())), with_kwargs=True)
                 for l, t in enumerate(m.transformers)]
        r = min(tc.TAP_ROWS, len(c["src"]))
        m.set_neighbor_sampler(sampler)                                  # resets a random sampler's state
        m.compute_src_dst_node_temporal_embeddings(c["src"][:r], c["dst"][:r], c["times"][:r], num_neighbors=K)
        for h in hooks:
            h.remove()
    assert all(len(x) == 4 for x in calls)
    out["tap_encoder_input"] = np.stack([calls[0][0][0], calls[0][1][0]], axis=1)
    out["tap_ids"] = np.stack([calls[0][0][1], calls[0][1][1]], axis=1).astype(np.int64)          # the self-attention masks: the sequences' own ids
    for l in range(layers):
        out[f"tap_layer_out_{l}"] = np.stack([calls[l][2][2], calls[l][3][2]], axis=1)
    assert np.isfinite(out["src_emb"]).all() and np.isfinite(out["src_neg_emb"]).all()
    print(f"{name}: max |emb| {np.abs(out['src_emb']).max():.3g}, max |src_pos - src_neg| {np.abs(out['src_emb'] - out['src_neg_emb']).max():.3g}")
    path = os.path.join(gc.GOLDEN_DIR, f"tcl_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


def make_eval():
    from evaluate_models_utils import evaluate_model_link_prediction
    from models.modules import MergeLayer
    from utils.DataLoader import Data, get_idx_data_loader
    from utils.utils import NegativeEdgeSampler
    c = tc.build_eval_case()
    cfg = c["tcl_cfg"]
    backbone, sampler = ref_model(c)
    merge = MergeLayer(172, 172, 172, 1)
    merge.load_state_dict({k: torch.from_numpy(v) for k, v in c["mparams"].items()}, strict=True)
    model = torch.nn.Sequential(backbone, merge)
    d = c["data"]
    a, b = gc.eval_indices(d.num_interactions)
    ev = Data(d.src_node_ids[a:b], d.dst_node_ids[a:b], d.node_interact_times[a:b], d.edge_ids[a:b], d.labels[a:b])
    neg = NegativeEdgeSampler(d.src_node_ids, d.dst_node_ids, seed=gc.EVAL_NEG_SEED)
    loader = get_idx_data_loader(list(range(b - a)), batch_size=cfg["batch"], shuffle=False)
    losses, metrics = evaluate_model_link_prediction("TCL", model, sampler, loader, neg, ev, torch.nn.BCELoss(), num_neighbors=cfg["K"])
    neg.reset_random_state()
    draws = np.concatenate([neg.sample(size=len(idx))[1] for idx in loader])
    path = os.path.join(gc.GOLDEN_DIR, "eval_tcl.npz")
    np.savez_compressed(path, losses=np.array(losses, dtype=np.float64), average_precision=np.array([m["average_precision"] for m in metrics]),
                        roc_auc=np.array([m["roc_auc"] for m in metrics]), neg_dst=draws.astype(np.int64))
    print(f"{path}: {os.path.getsize(path)} bytes, {len(losses)} batches")


if __name__ == "__main__":
    for name in tc.CASES:
        make_case(name)
    make_eval()
