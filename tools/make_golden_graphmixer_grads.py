"""Gradient fixtures of the GraphMixer tests, produced by the REFERENCE's own autograd: imports it from $DYGLIB_REFERENCE at run time
(nothing of it is copied), loads the seeded parameters of tests/graphmixer_cases.py with strict=True and, for every case below, runs the
model in eval mode (dropout is the identity) with autograd on:

    loss = sum(src_emb * G1) + sum(dst_emb * G2),   G1, G2 = tests.golden_cases.grad_loss_weights(B)

and writes tests/golden/grads_graphmixer_<case>.npz: the gradient of every parameter that has one (the time encoder is frozen and has none)
through tests.golden_cases.grad_signature (small tensors whole, big matrices as a corner and eight random projections), src_emb, dst_emb
and loss.

Only outputs are stored; the tests rebuild the inputs from the recipes.

    python tools/make_golden_graphmixer_grads.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tests import golden_cases as gc  # noqa: E402
from tests import graphmixer_cases as gmc  # noqa: E402
from make_golden_graphmixer import ref_model  # noqa: E402  (puts $DYGLIB_REFERENCE on sys.path)

# one block / two / three; G below, around and above the degrees; the last two have 7 and 10 roots with an empty history
GRAD_CASES = ("gen_k10_g7", "bip_k30_g50", "hub_k30_l3_g2000")


def make_case(name: str):
    c = gmc.build_graphmixer_case(name)
    cfg = c["gm_cfg"]
    m, _ = ref_model(c, cfg["K"], cfg["layers"])                          # eval mode
    s, d = m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=cfg["K"], time_gap=cfg["G"])
    G1, G2 = gc.grad_loss_weights(len(c["src"]))
    loss = (s * torch.from_numpy(G1)).sum() + (d * torch.from_numpy(G2)).sum()
    loss.backward()
    out = {"src_emb": s.detach().numpy(), "dst_emb": d.detach().numpy(), "loss": np.array(float(loss.detach()))}
    for k, p in m.named_parameters():
        if k.startswith("time_encoder."):
            assert p.grad is None and not p.requires_grad, k
            continue
        assert p.grad is not None and np.isfinite(p.grad.numpy()).all(), k
        out.update(gc.grad_signature(k, p.grad.numpy()))
    path = os.path.join(gc.GOLDEN_DIR, f"grads_graphmixer_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: loss {float(loss.detach()):.6g}, {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    for name in GRAD_CASES:
        make_case(name)
