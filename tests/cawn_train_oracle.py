"""Differentiable restatement of the CAWN TRAIN-mode forward (models/CAWN.py:48-396, TransformerEncoder models/modules.py:209-266): the
operations of tests/cawn_oracle.py with autograd on and the four dropout sites of the walk encoder's transformer block as multipliers from
oracle.dropout.Drop.mask(site, idx), indexed as dyglib_amd/csrc/cawn_train.hip documents:

    sequence index q = 2 p + side (side 0 = source), M walks per sequence, A = attention_dim, H heads
    site 0 (attention probabilities) element ((q H + h) M + i) M + j;   sites 1 (attention block output) and 3 (fc1 output) element
    (q M + i) A + c;   site 2 (relu(fc0)) element (q M + i) 4A + c

With p = 0 (drop = None) it is the eval-mode forward; drop = a float p draws the masks from torch's generator instead (plain PyTorch
dropout).  Test infrastructure: pinned to the reference's own gradients by tests/test_cawn_grads_cpu.py; the GPU tests and
tools/bench_cawn_train.py run the same operations (the latter on `cuda`); the product never imports it."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch
import torch.nn.functional as F

from oracle.dropout import Drop
from tests import cawn_oracle as co
from tests.tcl_train_oracle import _mask


def block(P: Dict[str, torch.Tensor], p: str, x: torch.Tensor, num_heads: int, drop, q_idx: torch.Tensor) -> torch.Tensor:
    """cawn_oracle.block with the four dropout sites; q_idx [n] = the pair-sequence index of the sequences"""
    n, S, d = x.shape
    dh = d // num_heads
    Wm, b = P[p + "multi_head_attention.in_proj_weight"], P[p + "multi_head_attention.in_proj_bias"]
    heads = lambda t: t.reshape(n, S, num_heads, dh).permute(0, 2, 1, 3)
    q = heads(F.linear(x, Wm[:d], b[:d])) * (1.0 / float(np.sqrt(dh)))
    k = heads(F.linear(x, Wm[d:2 * d], b[d:2 * d]))
    v = heads(F.linear(x, Wm[2 * d:], b[2 * d:]))
    pr = torch.softmax(q @ k.transpose(-1, -2), dim=-1)
    m = _mask(drop, 0, q_idx, (num_heads, S, S), pr)
    pr = pr if m is None else pr * m
    o = (pr @ v).permute(0, 2, 1, 3).reshape(n, S, d)
    o = F.linear(o, P[p + "multi_head_attention.out_proj.weight"], P[p + "multi_head_attention.out_proj.bias"])
    m = _mask(drop, 1, q_idx, (S, d), o)
    y = F.layer_norm(x + (o if m is None else o * m), (d,), P[p + "norm_layers.0.weight"], P[p + "norm_layers.0.bias"], 1e-5)
    hid = F.relu(F.linear(y, P[p + "linear_layers.0.weight"], P[p + "linear_layers.0.bias"]))
    m = _mask(drop, 2, q_idx, (S, 4 * d), hid)
    h = F.linear(hid if m is None else hid * m, P[p + "linear_layers.1.weight"], P[p + "linear_layers.1.bias"])
    m = _mask(drop, 3, q_idx, (S, d), h)
    return F.layer_norm(y + (h if m is None else h * m), (d,), P[p + "norm_layers.1.weight"], P[p + "norm_layers.1.bias"], 1e-5)


def encode_side(P, node_feat, edge_feat, roots, times, hops, levels_a, levels_b, num_heads: int, drop, q_idx):
    """cawn_oracle.encode_side with the block above"""
    k = hops[0][0].shape[1]
    levels = co.tree_levels(roots, hops)
    mlp = lambda t: F.linear(F.relu(F.linear(t, P["position_encoder.position_encode_layer.0.weight"], P["position_encoder.position_encode_layer.0.bias"])),
                             P["position_encoder.position_encode_layer.2.weight"], P["position_encoder.position_encode_layer.2.bias"])
    xs, ps = [], []
    for lv, ids in enumerate(levels):
        eids = torch.zeros_like(ids) if lv == 0 else hops[lv - 1][1]
        tn = times.unsqueeze(1) if lv == 0 else hops[lv - 1][2].double()
        dt = (times.unsqueeze(1) - tn).float()
        tf = torch.cos((dt.double().unsqueeze(-1) * P["time_encoder.w.weight"].reshape(1, 1, -1).double() + P["time_encoder.w.bias"].double()).float())
        pos = mlp(co.counts(levels_a, levels_b, ids)).sum(dim=-2)
        ps.append(pos)
        xs.append(torch.cat([node_feat[ids], tf, edge_feat[eids], pos], dim=-1))
    valid = [ids != 0 for ids in levels]
    fo = co.bilstm_last(P, "walk_encoder.feature_encoder.bilstm_encoder.", xs, valid, k)
    po = co.bilstm_last(P, "walk_encoder.position_encoder.bilstm_encoder.", ps, valid, k)
    x = F.linear(torch.cat([fo, po], dim=-1), P["walk_encoder.projection_layers.0.weight"], P["walk_encoder.projection_layers.0.bias"])
    y = block(P, "walk_encoder.transformer_encoder.", x, num_heads, drop, q_idx)
    return F.linear(y.mean(dim=-2), P["walk_encoder.projection_layers.1.weight"], P["walk_encoder.projection_layers.1.bias"])


def forward(P, node_feat, edge_feat, src, dst, times, src_hops, dst_hops, num_heads: int, drop=None):
    """tensors in, tensors out (any device): (src_emb, dst_emb) with a graph"""
    la, lb = co.tree_levels(src, src_hops), co.tree_levels(dst, dst_hops)
    qa = 2 * torch.arange(src.shape[0], dtype=torch.int64)
    a = encode_side(P, node_feat, edge_feat, src, times, src_hops, la, lb, num_heads, drop, qa)
    b = encode_side(P, node_feat, edge_feat, dst, times, dst_hops, la, lb, num_heads, drop, qa + 1)
    return a, b


def cawn_train_forward(P: Dict[str, torch.Tensor], node_feat, edge_feat, src, dst, times, src_graphs, dst_graphs, num_heads: int,
                       dropout_p: float = 0.0, seed: int = 0):
    """compute_src_dst_node_temporal_embeddings in train mode on sampled hops.  P: parameter tensors (requires_grad as the caller wishes, on
    any device); the other arguments are numpy arrays as in cawn_oracle.cawn_forward -> (src_emb, dst_emb) tensors [n, F_n] with a graph."""
    dev = next(iter(P.values())).device
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)
    hops = lambda g: [(t(n, np.int64), t(e, np.int64), t(ts, np.float32)) for n, e, ts in zip(*g)]
    drop = Drop(dropout_p, seed) if dropout_p > 0 else None
    return forward(P, t(node_feat, np.float32), t(edge_feat, np.float32), t(src, np.int64), t(dst, np.int64), t(times, np.float64), hops(src_graphs),
                   hops(dst_graphs), num_heads, drop)
