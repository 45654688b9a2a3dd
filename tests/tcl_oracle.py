"""CPU restatement of the reference TCL forward in eval mode (models/TCL.py:56-154, TransformerEncoder models/modules.py:209-266): test
infrastructure, pinned against the reference's own outputs by tests/test_tcl_oracle_golden.py.  Plain float32 array operations (torch
tensors, so that tools/bench_tcl.py can run the same operations on a GPU), attention written out: no nn.MultiheadAttention.  It takes the
SAMPLED neighbour arrays, so every sampling strategy is covered by whoever samples.  The GPU tests compare with it at shapes that have no
fixture; the product never imports it."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F


def encoder_input(P: Dict[str, torch.Tensor], node_feat: torch.Tensor, edge_feat: torch.Tensor, roots: torch.Tensor, times: torch.Tensor,
                  nbr: torch.Tensor, eid: torch.Tensor, ts: torch.Tensor):
    """roots [n] int64, times [n] float64, nbr / eid [n, K] int64, ts [n, K] float32 -> (ids [n, S] int64, x [n, S, d]): position 0 is the
    root (edge id 0, time = the query time), a padded slot reads node row 0, edge row 0 and dt = t - 0."""
    ids = torch.cat([roots.unsqueeze(1), nbr], dim=1)
    eids = torch.cat([torch.zeros_like(roots).unsqueeze(1), eid], dim=1)
    dt = (times.unsqueeze(1) - torch.cat([times.unsqueeze(1), ts.double()], dim=1)).float()      # float64 - float32 -> float64 -> .float()
    # the K = 1 Linear of the time encoder as ONE fused multiply-add (oracle.dygformer_oracle.time_encode): float32(float64(dt) * w + b)
    tf = torch.cos((dt.double().unsqueeze(-1) * P["time_encoder.w.weight"].reshape(1, 1, -1).double() + P["time_encoder.w.bias"].double()).float())
    lin = lambda x, k: F.linear(x, P[f"projection_layer.{k}.weight"], P[f"projection_layer.{k}.bias"])
    x = lin(node_feat[ids], "node") + lin(edge_feat[eids], "edge") + lin(tf, "time") + P["depth_embedding.weight"][:ids.shape[1]]
    return ids, x


def block(P: Dict[str, torch.Tensor], l: int, xq: torch.Tensor, xkv: torch.Tensor, key_ids: torch.Tensor, num_heads: int) -> torch.Tensor:
    """transformers[l](inputs_query = xq [n, Sq, d], inputs_key = inputs_value = xkv [n, Sk, d], neighbor_masks = key_ids [n, Sk])."""
    p = f"transformers.{l}."
    n, Sq, d = xq.shape
    Sk, dh = xkv.shape[1], d // num_heads
    W, b = P[p + "multi_head_attention.in_proj_weight"], P[p + "multi_head_attention.in_proj_bias"]
    heads = lambda x, S: x.reshape(n, S, num_heads, dh).permute(0, 2, 1, 3)
    q = heads(F.linear(xq, W[:d], b[:d]), Sq) * (1.0 / float(np.sqrt(dh)))
    k = heads(F.linear(xkv, W[d:2 * d], b[d:2 * d]), Sk)
    v = heads(F.linear(xkv, W[2 * d:], b[2 * d:]), Sk)
    s = (q @ k.transpose(-1, -2)).masked_fill((key_ids == 0).reshape(n, 1, 1, Sk), float("-inf"))
    o = (torch.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).reshape(n, Sq, d)
    o = F.linear(o, P[p + "multi_head_attention.out_proj.weight"], P[p + "multi_head_attention.out_proj.bias"])
    y = F.layer_norm(xq + o, (d,), P[p + "norm_layers.0.weight"], P[p + "norm_layers.0.bias"], 1e-5)
    h = F.linear(F.relu(F.linear(y, P[p + "linear_layers.0.weight"], P[p + "linear_layers.0.bias"])), P[p + "linear_layers.1.weight"],
                 P[p + "linear_layers.1.bias"])
    return F.layer_norm(y + h, (d,), P[p + "norm_layers.1.weight"], P[p + "norm_layers.1.bias"], 1e-5)


def layers(P: Dict[str, torch.Tensor], ids_a, xa, ids_b, xb, num_layers: int, num_heads: int, taps: Optional[dict] = None):
    """models/TCL.py:130-152 -> (out_a, out_b) [n, d]"""
    for l in range(num_layers):
        ya = block(P, l, xa, xa, ids_a, num_heads)
        yb = block(P, l, xb, xb, ids_b, num_heads)
        xa, xb = block(P, l, ya, yb, ids_b, num_heads), block(P, l, yb, ya, ids_a, num_heads)
        if taps is not None:
            taps["layer_out"].append(torch.stack([xa, xb], dim=1))
    out = lambda x: F.linear(x[:, 0, :], P["output_layer.weight"], P["output_layer.bias"])
    return out(xa), out(xb)


def tcl_forward(params: Dict[str, np.ndarray], node_feat: np.ndarray, edge_feat: np.ndarray, src: np.ndarray, dst: np.ndarray, times: np.ndarray,
                src_nbrs, dst_nbrs, num_layers: int, num_heads: int, taps: bool = False):
    """compute_src_dst_node_temporal_embeddings on sampled neighbours: src_nbrs / dst_nbrs = (ids, edge ids [n, K] int64, times [n, K] float32)
    as get_historical_neighbors returns them -> (src_emb, dst_emb) float32 [n, d] (numpy); with taps also dict(encoder_input [n, 2, S, d],
    layer_out: per layer [n, 2, S, d])."""
    P = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for k, v in params.items()}
    nf, ef = torch.from_numpy(np.ascontiguousarray(node_feat, dtype=np.float32)), torch.from_numpy(np.ascontiguousarray(edge_feat, dtype=np.float32))
    tms = torch.from_numpy(np.asarray(times, dtype=np.float64))
    side = lambda roots, nb: encoder_input(P, nf, ef, torch.from_numpy(np.asarray(roots, dtype=np.int64)), tms,
                                           torch.from_numpy(np.asarray(nb[0], dtype=np.int64)), torch.from_numpy(np.asarray(nb[1], dtype=np.int64)),
                                           torch.from_numpy(np.asarray(nb[2], dtype=np.float32)))
    with torch.no_grad():
        ids_a, xa = side(src, src_nbrs)
        ids_b, xb = side(dst, dst_nbrs)
        tp = dict(encoder_input=torch.stack([xa, xb], dim=1), layer_out=[]) if taps else None
        a, b = layers(P, ids_a, xa, ids_b, xb, num_layers, num_heads, tp)
    if not taps:
        return a.numpy(), b.numpy()
    return a.numpy(), b.numpy(), dict(encoder_input=tp["encoder_input"].numpy(), layer_out=[x.numpy() for x in tp["layer_out"]],
                                      ids=np.stack([ids_a.numpy(), ids_b.numpy()], axis=1))


def valid(ids: np.ndarray) -> np.ndarray:
    """[n, 2, S] node ids -> the mask of the positions whose values are specified (padded positions are not)"""
    return np.asarray(ids) != 0


def sample_uniform(adj, node_ids: np.ndarray, times: np.ndarray, k: int, random_state: np.random.RandomState):
    """utils/utils.py:149-214, `uniform` branch on a seeded sampler (:187-199): k draws with replacement from the history, re-sorted by the
    float32 times with numpy's default (unstable, but deterministic) argsort.  Consumes `random_state` row by row."""
    from oracle.dygformer_oracle import find_neighbors_before
    out_n = np.zeros((len(node_ids), k), dtype=np.int64)
    out_e = np.zeros((len(node_ids), k), dtype=np.int64)
    out_t = np.zeros((len(node_ids), k), dtype=np.float32)
    for r, (node, t) in enumerate(zip(node_ids, times)):
        nbr, eid, ts = find_neighbors_before(adj, node, t)
        if len(nbr) > 0:
            sampled = random_state.choice(a=len(nbr), size=k)
            out_t[r, :] = ts[sampled]
            pos = out_t[r, :].argsort()
            out_n[r, :], out_e[r, :], out_t[r, :] = nbr[sampled][pos], eid[sampled][pos], out_t[r, :][pos]
    return out_n, out_e, out_t
