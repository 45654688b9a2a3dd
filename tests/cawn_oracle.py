"""CPU restatement of the reference CAWN forward in eval mode (models/CAWN.py:48-396, TransformerEncoder models/modules.py:209-266): test
infrastructure, pinned against the reference's own outputs by tests/test_cawn_cpu.py.  Plain float32 array operations (torch tensors, so
that tools/bench_cawn.py can run the same operations on a GPU); no nn.LSTM, no packed sequences, no nn.MultiheadAttention.  It takes the
SAMPLED hop arrays, so every sampling strategy is covered by whoever samples.  Two rewrites of the reference are stated here, and proved by
the fixtures:

  * the reverse direction of a BiLSTM, read at the last valid position of a walk, is ONE cell on that position from the zero state;
  * position 0 of the M walks of a side is one row (the target, dt = 0, edge row 0, the target's position feature), so the forward
    direction's step 0 is computed once per side; step h once per hop-h node of the tree.

The product never imports this module."""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np
import torch
import torch.nn.functional as F

Hops = List[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]      # per hop h = 1..W: ids, edge ids [n, k^h] int64, times [n, k^h] float32


def tree_levels(roots: torch.Tensor, hops: Hops) -> List[torch.Tensor]:
    """node ids per level: [n, 1], [n, k], [n, k^2]"""
    return [roots.unsqueeze(1)] + [h[0] for h in hops]


def counts(levels_a: List[torch.Tensor], levels_b: List[torch.Tensor], x: torch.Tensor) -> torch.Tensor:
    """models/CAWN.py:197-256 for the node ids x [n, m] of pairs whose trees are levels_a / levels_b -> [n, m, 2, W + 1]: row 0 / 1 the
    landing probabilities in a's / b's tree (appearances at hop h over k^h); the entry of id 0 is zero."""
    rows = []
    for levels in (levels_a, levels_b):
        rows.append(torch.stack([(lv.unsqueeze(1) == x.unsqueeze(2)).sum(-1).float() / float(lv.shape[1]) for lv in levels], dim=-1))
    c = torch.stack(rows, dim=2)
    return c * (x != 0).reshape(x.shape + (1, 1)).float()


def lstm_cell(P: Dict[str, torch.Tensor], prefix: str, suffix: str, x: torch.Tensor, h: torch.Tensor = None, c: torch.Tensor = None):
    """one nn.LSTM step (gates i, f, g, o); h = c = None is the zero state: no hidden-state product"""
    g = F.linear(x, P[prefix + "weight_ih_l0" + suffix], P[prefix + "bias_ih_l0" + suffix]) + P[prefix + "bias_hh_l0" + suffix]
    if h is not None:
        g = g + F.linear(h, P[prefix + "weight_hh_l0" + suffix])
    i, f, gg, o = g.chunk(4, dim=-1)
    cn = torch.sigmoid(i) * torch.tanh(gg)
    if c is not None:
        cn = cn + torch.sigmoid(f) * c
    return torch.sigmoid(o) * torch.tanh(cn), cn


def bilstm_last(P: Dict[str, torch.Tensor], prefix: str, xs: List[torch.Tensor], valid: List[torch.Tensor], k: int) -> torch.Tensor:
    """models/CAWN.py:371-396 on the tree: xs[h] [n, k^h, in] the inputs of the level-h nodes, valid[h] [n, k^h] -> [n, M, 2 H], the BiLSTM's
    output at the last valid position of every walk."""
    W, M = len(xs) - 1, xs[-1].shape[1]
    h, c = lstm_cell(P, prefix, "", xs[0])                                           # step 0: once per side
    rev = lstm_cell(P, prefix, "_reverse", xs[0])[0].expand(-1, M, -1)
    for lv in range(1, W + 1):
        hp, cp = h.repeat_interleave(k, dim=1), c.repeat_interleave(k, dim=1)      # the parent's state
        hn, cn = lstm_cell(P, prefix, "", xs[lv], hp, cp)
        on = valid[lv].unsqueeze(-1)
        h, c = torch.where(on, hn, hp), torch.where(on, cn, cp)                      # a walk that ended keeps its state
        up = lambda t: t.repeat_interleave(M // t.shape[1], dim=1)
        rev = torch.where(up(on), up(lstm_cell(P, prefix, "_reverse", xs[lv])[0]), rev)      # the deepest valid level wins
    return torch.cat([h, rev], dim=-1)


def block(P: Dict[str, torch.Tensor], p: str, x: torch.Tensor, num_heads: int) -> torch.Tensor:
    """the TransformerEncoder p on x [n, S, d], self-attention without a mask"""
    n, S, d = x.shape
    dh = d // num_heads
    Wm, b = P[p + "multi_head_attention.in_proj_weight"], P[p + "multi_head_attention.in_proj_bias"]
    heads = lambda t: t.reshape(n, S, num_heads, dh).permute(0, 2, 1, 3)
    q = heads(F.linear(x, Wm[:d], b[:d])) * (1.0 / float(np.sqrt(dh)))
    k = heads(F.linear(x, Wm[d:2 * d], b[d:2 * d]))
    v = heads(F.linear(x, Wm[2 * d:], b[2 * d:]))
    o = (torch.softmax(q @ k.transpose(-1, -2), dim=-1) @ v).permute(0, 2, 1, 3).reshape(n, S, d)
    o = F.linear(o, P[p + "multi_head_attention.out_proj.weight"], P[p + "multi_head_attention.out_proj.bias"])
    y = F.layer_norm(x + o, (d,), P[p + "norm_layers.0.weight"], P[p + "norm_layers.0.bias"], 1e-5)
    h = F.linear(F.relu(F.linear(y, P[p + "linear_layers.0.weight"], P[p + "linear_layers.0.bias"])), P[p + "linear_layers.1.weight"],
                 P[p + "linear_layers.1.bias"])
    return F.layer_norm(y + h, (d,), P[p + "norm_layers.1.weight"], P[p + "norm_layers.1.bias"], 1e-5)


def encode_side(P: Dict[str, torch.Tensor], node_feat, edge_feat, roots, times, hops: Hops, levels_a, levels_b, num_heads: int, taps: dict = None):
    """compute_node_temporal_embeddings (models/CAWN.py:82-128) of the sides (roots, times, hops) paired as the trees levels_a / levels_b"""
    n, k, W = roots.shape[0], hops[0][0].shape[1], len(hops)
    M = k ** W
    levels = tree_levels(roots, hops)
    mlp = lambda t: F.linear(F.relu(F.linear(t, P["position_encoder.position_encode_layer.0.weight"], P["position_encoder.position_encode_layer.0.bias"])),
                             P["position_encoder.position_encode_layer.2.weight"], P["position_encoder.position_encode_layer.2.bias"])
    xs, ps, cs = [], [], []
    for lv, ids in enumerate(levels):
        eids = torch.zeros_like(ids) if lv == 0 else hops[lv - 1][1]
        tn = times.unsqueeze(1) if lv == 0 else hops[lv - 1][2].double()
        dt = (times.unsqueeze(1) - tn).float()                                       # float64 - float32 -> float64 -> .float()
        tf = torch.cos((dt.double().unsqueeze(-1) * P["time_encoder.w.weight"].reshape(1, 1, -1).double() + P["time_encoder.w.bias"].double()).float())
        c = counts(levels_a, levels_b, ids)                                           # [n, k^lv, 2, W + 1]
        pos = mlp(c).sum(dim=-2)                                                      # once per tree node, both rows summed (:288)
        cs.append(c), ps.append(pos)
        xs.append(torch.cat([node_feat[ids], tf, edge_feat[eids], pos], dim=-1))      # models/CAWN.py:342
    valid = [ids != 0 for ids in levels]
    fo = bilstm_last(P, "walk_encoder.feature_encoder.bilstm_encoder.", xs, valid, k)
    po = bilstm_last(P, "walk_encoder.position_encoder.bilstm_encoder.", ps, valid, k)
    x = F.linear(torch.cat([fo, po], dim=-1), P["walk_encoder.projection_layers.0.weight"], P["walk_encoder.projection_layers.0.bias"])
    y = block(P, "walk_encoder.transformer_encoder.", x, num_heads)
    out = F.linear(y.mean(dim=-2), P["walk_encoder.projection_layers.1.weight"], P["walk_encoder.projection_layers.1.bias"])
    if taps is not None:
        up = lambda t: t.repeat_interleave(M // t.shape[1], dim=1)
        taps["walk_ids"].append(torch.stack([up(ids) for ids in levels], dim=2))
        taps["counts"].append(torch.stack([up(c) for c in cs], dim=2))
        taps["feature_out"].append(fo), taps["position_out"].append(po), taps["attn_in"].append(x), taps["attn_out"].append(y)
    return out


TAP_KEYS = ("walk_ids", "counts", "feature_out", "position_out", "attn_in", "attn_out")


def forward(P, node_feat, edge_feat, src, dst, times, src_hops: Hops, dst_hops: Hops, num_heads: int, taps: bool = False):
    """tensors in, tensors out (any device): (src_emb, dst_emb[, taps with index 0 / 1 of the second axis = source / destination])"""
    la, lb = tree_levels(src, src_hops), tree_levels(dst, dst_hops)
    tp = {k: [] for k in TAP_KEYS} if taps else None
    a = encode_side(P, node_feat, edge_feat, src, times, src_hops, la, lb, num_heads, tp)
    b = encode_side(P, node_feat, edge_feat, dst, times, dst_hops, la, lb, num_heads, tp)
    return (a, b) if not taps else (a, b, {k: torch.stack(v, dim=1) for k, v in tp.items()})


def cawn_forward(params: Dict[str, np.ndarray], node_feat: np.ndarray, edge_feat: np.ndarray, src: np.ndarray, dst: np.ndarray, times: np.ndarray,
                 src_graphs, dst_graphs, num_heads: int, taps: bool = False):
    """compute_src_dst_node_temporal_embeddings on sampled hops: src_graphs / dst_graphs = (ids per hop, edge ids per hop, times per hop) as
    get_multi_hop_neighbors returns them -> numpy (src_emb, dst_emb[, taps])."""
    P = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for k, v in params.items()}
    nf, ef = torch.from_numpy(np.ascontiguousarray(node_feat, dtype=np.float32)), torch.from_numpy(np.ascontiguousarray(edge_feat, dtype=np.float32))
    i64 = lambda x: torch.from_numpy(np.asarray(x, dtype=np.int64))
    hops = lambda g: [(i64(n), i64(e), torch.from_numpy(np.asarray(t, dtype=np.float32))) for n, e, t in zip(*g)]
    with torch.no_grad():
        out = forward(P, nf, ef, i64(src), i64(dst), torch.from_numpy(np.asarray(times, dtype=np.float64)), hops(src_graphs), hops(dst_graphs), num_heads, taps)
    if not taps:
        return out[0].numpy(), out[1].numpy()
    return out[0].numpy(), out[1].numpy(), {k: v.numpy() for k, v in out[2].items()}


class OracleSampler:
    """The reference's sampler calls restated on the host (utils/utils.py:112-128, :149-252) for the three strategies; a random strategy draws
    from ONE RandomState that carries over from call to call, row by row."""

    def __init__(self, data, strategy: str, seed: int, time_scaling_factor: float = 0.0):
        from oracle import dygformer_oracle as orc
        self.orc = orc
        self.adj = orc.OracleAdjacency(data.src_node_ids, data.dst_node_ids, data.edge_ids, data.node_interact_times)
        self.strategy, self.seed, self.scale = strategy, seed, time_scaling_factor
        self.reset()

    def reset(self):
        self.rs = np.random.RandomState(self.seed)

    def probabilities(self, node: int, n: int):
        """time_interval_aware: exp(scale (t - t_last)) over its running sum on the node's WHOLE history, cut to the first n, softmax in float32"""
        ts = self.adj.row(int(node))[2]
        e = np.exp(self.scale * (ts - np.max(ts)))
        with np.errstate(divide="ignore", invalid="ignore"):
            p = e / np.cumsum(e)
        p[np.isnan(p)] = -1e10
        return torch.softmax(torch.from_numpy(p[:n]).float(), dim=0).numpy()

    def __call__(self, ids: np.ndarray, times: np.ndarray, k: int):
        if self.strategy == "recent":
            return self.orc.get_historical_neighbors_recent(self.adj, ids, times, k)
        out_n, out_e = np.zeros((len(ids), k), dtype=np.int64), np.zeros((len(ids), k), dtype=np.int64)
        out_t = np.zeros((len(ids), k), dtype=np.float32)
        for r, (node, t) in enumerate(zip(ids, times)):
            nbr, eid, ts = self.orc.find_neighbors_before(self.adj, node, t)
            if len(nbr) == 0:
                continue
            p = self.probabilities(node, len(nbr)) if self.strategy == "time_interval_aware" else None
            drawn = self.rs.choice(a=len(nbr), size=k, p=p)
            out_t[r] = ts[drawn]
            pos = out_t[r].argsort()                                     # on the float32 times, numpy's default sort
            out_n[r], out_e[r], out_t[r] = nbr[drawn][pos], eid[drawn][pos], out_t[r][pos]
        return out_n, out_e, out_t

    def multi_hop(self, num_hops: int, ids: np.ndarray, times: np.ndarray, k: int):
        """hop h >= 2 queries every hop h - 1 node at its float32 time -> (ids per hop, edge ids per hop, times per hop), [n, k^h] each"""
        n, e, t = self(ids, times, k)
        out = ([n], [e], [t])
        for _ in range(1, num_hops):
            n, e, t = self(out[0][-1].flatten(), out[2][-1].flatten(), k)
            for lst, x in zip(out, (n, e, t)):
                lst.append(x.reshape(len(ids), -1))
        return out
