"""Gradient fixtures of the CAWN tests, produced by the REFERENCE's own autograd: imports it from $DYGLIB_REFERENCE at run time (nothing of it
is copied), loads the seeded parameters of tests/cawn_cases.py with strict=True and, for every case, runs the model in eval mode (dropout is
the identity) with autograd on:

    loss = sum(src_emb * G1) + sum(dst_emb * G2),   G1, G2 = tests.golden_cases.grad_loss_weights(B)

and writes tests/golden/grads_cawn_<case>.npz: every parameter's gradient through tests.golden_cases.grad_signature (small tensors whole,
big matrices as a corner and eight random projections), src_emb, dst_emb and loss.  For the two random-strategy cases also the embeddings of
a following no_grad call on (src, neg_dst) with the SAME sampler: its RandomState has been consumed by the first call.

Only outputs are stored; the tests rebuild the inputs from the recipes.

    DYGLIB_REFERENCE=<checkout of the reference> python tools/make_golden_cawn_grads.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tests import cawn_cases as cc  # noqa: E402
from tests import golden_cases as gc  # noqa: E402
from make_golden_cawn import ref_model  # noqa: E402  (puts $DYGLIB_REFERENCE on sys.path)


def make_case(name: str):
    c = cc.build_cawn_case(name)
    cfg = c["cawn_cfg"]
    k = cfg["k"]
    m, sampler = ref_model(c)                                            # eval mode
    m.set_neighbor_sampler(sampler)
    s, d = m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=k)
    G1, G2 = gc.grad_loss_weights(len(c["src"]))
    loss = (s * torch.from_numpy(G1)).sum() + (d * torch.from_numpy(G2)).sum()
    loss.backward()
    out = {"src_emb": s.detach().numpy(), "dst_emb": d.detach().numpy(), "loss": np.array(float(loss.detach()))}
    for key, p in m.named_parameters():
        assert p.grad is not None and np.isfinite(p.grad.numpy()).all(), key
        out.update(gc.grad_signature(key, p.grad.numpy()))
    if cfg["strategy"] != "recent":
        with torch.no_grad():
            sn, nd = m.compute_src_dst_node_temporal_embeddings(c["src"], c["neg_dst"], c["times"], num_neighbors=k)
        out["src_neg_emb"], out["neg_dst_emb"] = sn.numpy(), nd.numpy()
    path = os.path.join(gc.GOLDEN_DIR, f"grads_cawn_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: loss {float(loss.detach()):.6g}, {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    for name in (sys.argv[1:] or cc.CASES):
        make_case(name)
