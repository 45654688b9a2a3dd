#!/usr/bin/env python3
"""Gradient fixtures of the REFERENCE TGAT (models/TGAT.py) for the training path: tests/golden/grads_tgat_<case>.npz.  Run where the
reference is importable (the build container), like oracle/make_golden.py, whose reference bindings it reuses:

    python tools/make_golden_tgat_grads.py          # writes tests/golden/grads_tgat_*.npz

Per gc.TGAT_CASES case: the reference in eval mode (dropout is the identity) with autograd on, loss = sum(src_emb * G1) + sum(dst_emb * G2)
(G1, G2 = gc.grad_loss_weights(B)); every parameter gradient stored through gc.grad_signature, as run_grad_case does for DyGFormer.
grads_tgat_uniform_tgat_bip_l2_k20.npz: the same on a `uniform` sampler (gc.SAMPLING_STRATEGIES["uniform"]), then the embeddings of a following
no_grad negative call on the SAME sampler: they show that the gradient call consumed the sampler's RandomState exactly as the reference does.
Only outputs are stored; the inputs are rebuilt from the recipes."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as mg          # noqa: E402  (binds the reference classes)
from tests import golden_cases as gc          # noqa: E402

UNIFORM_CASE = "tgat_bip_l2_k20"


def _model(c, strategy="recent", seed=1, tsf=0.0):
    d, cfg = c["data"], c["tgat_cfg"]
    ref_data = mg.RefData(d.src_node_ids, d.dst_node_ids, d.node_interact_times, d.edge_ids, d.labels)
    sampler = mg.ref_get_neighbor_sampler(ref_data, sample_neighbor_strategy=strategy, time_scaling_factor=tsf, seed=seed)
    model = mg.RefTGAT(c["node_feat"], c["edge_feat"], sampler, time_feat_dim=cfg["time_feat_dim"], num_layers=cfg["num_layers"],
                       num_heads=cfg["num_heads"], dropout=0.1, device="cpu")
    r = model.load_state_dict({k: torch.from_numpy(v) for k, v in c["tgat_params"].items()}, strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    return model.eval()


def _grads(model, c) -> dict:
    k = c["tgat_cfg"]["num_neighbors"]
    se, de = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=k)
    G1, G2 = gc.grad_loss_weights(len(c["src"]))
    loss = (se * torch.from_numpy(G1)).sum() + (de * torch.from_numpy(G2)).sum()
    loss.backward()
    out = {"loss": np.array(float(loss.detach())), "src_emb": se.detach().numpy(), "dst_emb": de.detach().numpy()}
    for name, p in model.named_parameters():
        out.update(gc.grad_signature(name, p.grad.numpy()))
    return out


def run_case(name: str) -> dict:
    c = gc.build_tgat_case(name)
    return _grads(_model(c), c)


def run_uniform_case(name: str) -> dict:
    c = gc.build_tgat_case(name)
    strategy, seed, tsf = gc.SAMPLING_STRATEGIES["uniform"]
    model = _model(c, strategy, seed, tsf)
    out = _grads(model, c)
    with torch.no_grad():
        nse, nde = model.compute_src_dst_node_temporal_embeddings(c["src"], c["neg_dst"], c["times"], num_neighbors=c["tgat_cfg"]["num_neighbors"])
    out["neg_src_emb"], out["neg_dst_emb"] = nse.numpy(), nde.numpy()
    return out


def main():
    torch.set_num_threads(8)
    jobs = [("grads_" + n, run_case, n) for n in gc.TGAT_CASES] + [("grads_tgat_uniform_" + UNIFORM_CASE, run_uniform_case, UNIFORM_CASE)]
    for fname, fn, case in jobs:
        path = os.path.join(gc.GOLDEN_DIR, fname + ".npz")
        np.savez_compressed(path, **fn(case))
        print(f"{fname}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
