"""Differentiable restatement of the TCL TRAIN-mode forward (models/TCL.py:56-154, TransformerEncoder models/modules.py:209-266): the
operations of tests/tcl_oracle.py with autograd on and the four dropout sites of a block as multipliers from oracle.dropout.Drop.mask(site,
idx), indexed as dyglib_amd/csrc/tcl_train.hip documents:

    site = 8 layer + 4 stage + {0: attention probabilities, 1: attention block output, 2: relu(fc0), 3: fc1 output}; stage 0 = self, 1 = cross
    sequence index q = 2 p + side (side 0 = source), also in the self stage
    site 0 element ((q H + h) S + i) S + j;   sites 1, 3 element (q S + i) d + c;   site 2 element (q S + i) 4d + c

With p = 0 (drop = None) it is the eval-mode forward; drop = a float p draws the masks from torch's generator instead (plain PyTorch
dropout).  Test infrastructure: pinned to the reference's own gradients by tests/test_tcl_grads_cpu.py; the GPU tests and
tools/bench_tcl_train.py run the same operations (the latter on `cuda`); the product never imports it."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle.dropout import Drop
from tests import tcl_oracle as tco


def _mask(drop, site: int, q: torch.Tensor, shape, like: torch.Tensor):
    """The multipliers of a [n, *shape] activation whose rows belong to the pair sequences q [n]: element index q * prod(shape) + offset."""
    if drop is None:
        return None
    if isinstance(drop, float):          # plain PyTorch dropout (tools/bench_tcl_train.py): masks from torch's generator on the activation's device
        return torch.empty((len(q),) + tuple(shape), device=like.device).bernoulli_(1.0 - drop) / (1.0 - drop)
    per = int(np.prod(shape))
    idx = q.cpu().numpy().astype(np.int64).reshape(-1, 1) * per + np.arange(per, dtype=np.int64).reshape(1, -1)
    return torch.from_numpy(drop.mask(site, idx).reshape((len(q),) + tuple(shape))).to(like.device)


def block(P: Dict[str, torch.Tensor], l: int, stage: int, xq: torch.Tensor, xkv: torch.Tensor, key_ids: torch.Tensor, num_heads: int,
          drop: Optional[Drop], q_idx: torch.Tensor) -> torch.Tensor:
    """tcl_oracle.block with the four dropout sites; q_idx [n] = the pair-sequence index of the query sequences."""
    p = f"transformers.{l}."
    n, Sq, d = xq.shape
    Sk, dh = xkv.shape[1], d // num_heads
    site = 8 * l + 4 * stage
    W, b = P[p + "multi_head_attention.in_proj_weight"], P[p + "multi_head_attention.in_proj_bias"]
    heads = lambda x, S: x.reshape(n, S, num_heads, dh).permute(0, 2, 1, 3)
    q = heads(F.linear(xq, W[:d], b[:d]), Sq) * (1.0 / float(np.sqrt(dh)))
    k = heads(F.linear(xkv, W[d:2 * d], b[d:2 * d]), Sk)
    v = heads(F.linear(xkv, W[2 * d:], b[2 * d:]), Sk)
    s = (q @ k.transpose(-1, -2)).masked_fill((key_ids == 0).reshape(n, 1, 1, Sk), float("-inf"))
    pr = torch.softmax(s, dim=-1)
    m = _mask(drop, site, q_idx, (num_heads, Sq, Sk), pr)
    pr = pr if m is None else pr * m
    o = (pr @ v).permute(0, 2, 1, 3).reshape(n, Sq, d)
    o = F.linear(o, P[p + "multi_head_attention.out_proj.weight"], P[p + "multi_head_attention.out_proj.bias"])
    m = _mask(drop, site + 1, q_idx, (Sq, d), o)
    y = F.layer_norm(xq + (o if m is None else o * m), (d,), P[p + "norm_layers.0.weight"], P[p + "norm_layers.0.bias"], 1e-5)
    hid = F.relu(F.linear(y, P[p + "linear_layers.0.weight"], P[p + "linear_layers.0.bias"]))
    m = _mask(drop, site + 2, q_idx, (Sq, 4 * d), hid)
    h = F.linear(hid if m is None else hid * m, P[p + "linear_layers.1.weight"], P[p + "linear_layers.1.bias"])
    m = _mask(drop, site + 3, q_idx, (Sq, d), h)
    return F.layer_norm(y + (h if m is None else h * m), (d,), P[p + "norm_layers.1.weight"], P[p + "norm_layers.1.bias"], 1e-5)


def layers(P: Dict[str, torch.Tensor], ids_a, xa, ids_b, xb, num_layers: int, num_heads: int, drop: Optional[Drop] = None):
    """models/TCL.py:130-152 -> (out_a, out_b) [n, d]"""
    n = xa.shape[0]
    qa = 2 * torch.arange(n, dtype=torch.int64)
    qb = qa + 1
    for l in range(num_layers):
        ya = block(P, l, 0, xa, xa, ids_a, num_heads, drop, qa)
        yb = block(P, l, 0, xb, xb, ids_b, num_heads, drop, qb)
        xa, xb = block(P, l, 1, ya, yb, ids_b, num_heads, drop, qa), block(P, l, 1, yb, ya, ids_a, num_heads, drop, qb)
    out = lambda x: F.linear(x[:, 0, :], P["output_layer.weight"], P["output_layer.bias"])
    return out(xa), out(xb)


def tcl_train_forward(P: Dict[str, torch.Tensor], node_feat, edge_feat, src, dst, times, src_nbrs, dst_nbrs, num_layers: int, num_heads: int,
                      dropout_p: float = 0.0, seed: int = 0):
    """compute_src_dst_node_temporal_embeddings in train mode on sampled neighbours.  P: parameter tensors (requires_grad as the caller
    wishes, on any device); node_feat / edge_feat / src / dst / times / the neighbour triples: numpy arrays as in tcl_oracle.tcl_forward
    -> (src_emb, dst_emb) tensors [n, d] with a graph."""
    dev = next(iter(P.values())).device
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)
    nf, ef, tms = t(node_feat, np.float32), t(edge_feat, np.float32), t(times, np.float64)
    side = lambda roots, nb: tco.encoder_input(P, nf, ef, t(roots, np.int64), tms, t(nb[0], np.int64), t(nb[1], np.int64), t(nb[2], np.float32))
    ids_a, xa = side(src, src_nbrs)
    ids_b, xb = side(dst, dst_nbrs)
    drop = Drop(dropout_p, seed) if dropout_p > 0 else None
    return layers(P, ids_a, xa, ids_b, xb, num_layers, num_heads, drop)
