"""Fixtures of the GraphMixer tests, produced by the REFERENCE itself: imports it from $DYGLIB_REFERENCE at run time (nothing of it is
copied), loads the seeded parameters of tests/graphmixer_cases.py with strict=True, runs the eval-mode forward on the CPU and writes

    tests/golden/graphmixer_<case>.npz   embeddings of src / dst / neg_dst, the state_dict key list, and for the first TAP_ROWS source roots the
                                         projection output, every Mixer block's output, the token mean and the node-encoder term BEFORE
                                         node_feat[v] is added (captured with forward hooks and by recording the forward's two torch.mean
                                         results)
    tests/golden/eval_graphmixer.npz     per-batch loss / AP / AUC of the reference's evaluate_model_link_prediction and its negative draws

Only outputs are stored; the tests rebuild the inputs from the recipes.

    python tools/make_golden_graphmixer.py
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
from tests import graphmixer_cases as gmc  # noqa: E402


def ref_model(c, num_tokens, layers):
    from models.GraphMixer import GraphMixer
    from utils.DataLoader import Data
    from utils.utils import get_neighbor_sampler
    d = c["data"]
    sampler = get_neighbor_sampler(Data(d.src_node_ids, d.dst_node_ids, d.node_interact_times, d.edge_ids, d.labels), "recent", seed=1)
    m = GraphMixer(c["node_feat"], c["edge_feat"], sampler, gmc.TIME_FEAT_DIM, num_tokens=num_tokens, num_layers=layers, dropout=0.1)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["gm_params"].items()}, strict=True)
    return m.eval(), sampler


def make_case(name: str):
    c = gmc.build_graphmixer_case(name)
    K, layers, G = c["gm_cfg"]["K"], c["gm_cfg"]["layers"], c["gm_cfg"]["G"]
    m, _ = ref_model(c, K, layers)
    out = {"state_dict_keys": np.array(list(m.state_dict().keys()))}
    with torch.no_grad():
        s, d = m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=K, time_gap=G)
        _, nd = m.compute_src_dst_node_temporal_embeddings(c["src"], c["neg_dst"], c["times"], num_neighbors=K, time_gap=G)
        out["src_emb"], out["dst_emb"], out["neg_dst_emb"] = s.numpy(), d.numpy(), nd.numpy()
        cap = {}
        hooks = [m.projection_layer.register_forward_hook(lambda mod, i, o: cap.__setitem__("projection", o.detach().numpy().copy())),
                 m.output_layer.register_forward_hook(lambda mod, i, o: cap.__setitem__("cat", i[0].detach().numpy().copy()))]
        for l, mixer in enumerate(m.mlp_mixers):
            hooks.append(mixer.register_forward_hook(lambda mod, i, o, l=l: cap.__setitem__(f"layer_out_{l}", o.detach().numpy().copy())))
        r = min(gmc.TAP_ROWS, len(c["src"]))
        means, torch_mean = [], torch.mean
        torch.mean = lambda *a, **k: (means.append(torch_mean(*a, **k)), means[-1])[1]       # record what the forward's torch.mean calls return
        try:
            m.compute_node_temporal_embeddings(c["src"][:r], c["times"][:r], num_neighbors=K, time_gap=G)
        finally:
            torch.mean = torch_mean
        for h in hooks:
            h.remove()
    C = c["edge_feat"].shape[1]
    out["tap_projection"] = cap["projection"]
    for l in range(layers):
        out[f"tap_layer_out_{l}"] = cap[f"layer_out_{l}"]
    # the forward takes two means: over the tokens, then over the time_gap slots (the node-encoder term, before node_feat[v] is added);
    # output_layer's input [token mean | node term + node_feat[v]] identifies them
    assert len(means) == 2 and means[0].shape == (r, C) and means[1].shape == (r, c["node_feat"].shape[1])
    out["tap_token_mean"], out["tap_node_term"] = means[0].numpy(), means[1].numpy()
    assert np.array_equal(out["tap_token_mean"], cap["cat"][:, :C])
    assert np.array_equal((means[1] + torch.from_numpy(c["node_feat"][c["src"][:r]])).numpy(), cap["cat"][:, C:])
    path = os.path.join(gc.GOLDEN_DIR, f"graphmixer_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


def make_eval():
    from evaluate_models_utils import evaluate_model_link_prediction
    from models.modules import MergeLayer
    from utils.DataLoader import Data, get_idx_data_loader
    from utils.utils import NegativeEdgeSampler
    c = gmc.build_eval_case()
    cfg = c["gm_cfg"]
    backbone, sampler = ref_model(c, cfg["K"], cfg["layers"])
    merge = MergeLayer(172, 172, 172, 1)
    merge.load_state_dict({k: torch.from_numpy(v) for k, v in c["mparams"].items()}, strict=True)
    model = torch.nn.Sequential(backbone, merge)
    d = c["data"]
    a, b = gc.eval_indices(d.num_interactions)
    ev = Data(d.src_node_ids[a:b], d.dst_node_ids[a:b], d.node_interact_times[a:b], d.edge_ids[a:b], d.labels[a:b])
    neg = NegativeEdgeSampler(d.src_node_ids, d.dst_node_ids, seed=gc.EVAL_NEG_SEED)
    loader = get_idx_data_loader(list(range(b - a)), batch_size=cfg["batch"], shuffle=False)
    losses, metrics = evaluate_model_link_prediction("GraphMixer", model, sampler, loader, neg, ev, torch.nn.BCELoss(), num_neighbors=cfg["K"],
                                                     time_gap=cfg["G"])
    neg.reset_random_state()
    draws = np.concatenate([neg.sample(size=len(idx))[1] for idx in loader])
    path = os.path.join(gc.GOLDEN_DIR, "eval_graphmixer.npz")
    np.savez_compressed(path, losses=np.array(losses, dtype=np.float64), average_precision=np.array([m["average_precision"] for m in metrics]),
                        roc_auc=np.array([m["roc_auc"] for m in metrics]), neg_dst=draws.astype(np.int64))
    print(f"{path}: {os.path.getsize(path)} bytes, {len(losses)} batches")


if __name__ == "__main__":
    for name in gmc.CASES:
        make_case(name)
    make_eval()
