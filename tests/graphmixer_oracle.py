"""CPU restatement of the reference GraphMixer forward in eval mode (models/GraphMixer.py:70-150, MLPMixer :217-244) with `recent` sampling:
test infrastructure, pinned against the reference's own outputs by tests/test_graphmixer_oracle_golden.py.  float32 torch ops in the
reference's order where the order shows at 1e-4.  The GPU tests compare with it at shapes that have no fixture; the product never imports it.

`link_encoder`, `node_term_dense` and `output` take tensors on any device and the sampled neighbour arrays as arguments, so
tools/bench_graphmixer.py can time the same model in plain PyTorch ops on the GPU, fed by the package's own sampler."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle.dygformer_oracle import OracleAdjacency, find_neighbors_before, get_historical_neighbors_recent


def link_encoder(P: Dict[str, torch.Tensor], edge_feat: torch.Tensor, nbr: torch.Tensor, eid: torch.Tensor, dt: torch.Tensor, num_layers: int,
                 taps: Optional[dict] = None) -> torch.Tensor:
    """nbr / eid [n, K] int64, dt [n, K] float32 = float32(t - neighbour time) -> [n, C]: tokens [edge row | cos(w dt + b)], time half zero
    where the neighbour id is 0; projection; Mixer blocks; mean over the tokens."""
    # the K = 1 Linear of the time encoder as ONE fused multiply-add (see oracle.dygformer_oracle.time_encode: PyTorch's CPU addmm fuses it, and at
    # dt ~ 2.7e6 a float32 ulp is 0.25 rad): float32(float64(dt) * w + b), also on a GPU, where float64 is slow but exact
    tf = torch.cos((dt.double().unsqueeze(-1) * P["time_encoder.w.weight"].reshape(1, 1, -1).double() + P["time_encoder.w.bias"].double()).float())
    tf = tf.masked_fill((nbr == 0).unsqueeze(-1), 0.0)
    x = F.linear(torch.cat([edge_feat[eid], tf], dim=-1), P["projection_layer.weight"], P["projection_layer.bias"])
    if taps is not None:
        taps["projection"] = x
        taps["layer_out"] = []
    for l in range(num_layers):
        p = f"mlp_mixers.{l}."
        K, Cc = x.shape[1], x.shape[2]
        h = F.layer_norm(x.permute(0, 2, 1), (K,), P[p + "token_norm.weight"], P[p + "token_norm.bias"], 1e-5)
        h = F.gelu(F.linear(h, P[p + "token_feedforward.ffn.0.weight"], P[p + "token_feedforward.ffn.0.bias"]))
        h = F.linear(h, P[p + "token_feedforward.ffn.3.weight"], P[p + "token_feedforward.ffn.3.bias"])
        x = h.permute(0, 2, 1) + x
        h = F.layer_norm(x, (Cc,), P[p + "channel_norm.weight"], P[p + "channel_norm.bias"], 1e-5)
        h = F.gelu(F.linear(h, P[p + "channel_feedforward.ffn.0.weight"], P[p + "channel_feedforward.ffn.0.bias"]))
        x = F.linear(h, P[p + "channel_feedforward.ffn.3.weight"], P[p + "channel_feedforward.ffn.3.bias"]) + x
        if taps is not None:
            taps["layer_out"].append(x)
    m = x.mean(dim=1)
    if taps is not None:
        taps["token_mean"] = m
    return m


def node_term_dense(node_feat: torch.Tensor, nbr_gap: torch.Tensor) -> torch.Tensor:
    """The reference's formulation on the padded window nbr_gap [n, G]: softmax over a 1 / -1e10 mask (uniform over the valid slots; uniform
    over ALL slots when none is valid), weighted rows, torch.mean over the G slots.  Materialises [n, G, Fn]."""
    mask = (nbr_gap > 0).to(torch.float32)
    mask = torch.where(mask == 0, torch.full_like(mask, -1e10), mask)
    scores = torch.softmax(mask, dim=1)
    return torch.mean(node_feat[nbr_gap] * scores.unsqueeze(-1), dim=1)


def node_term_rows(node_feat: np.ndarray, adj: OracleAdjacency, node_ids: np.ndarray, times: np.ndarray, G: int) -> np.ndarray:
    """The same quantity root by root without the padded window: (1 / G) (1 / m) sum of the m = min(history, G) most recent neighbours' rows,
    node_feat[0] / G for m = 0."""
    out = np.empty((len(node_ids), node_feat.shape[1]), dtype=np.float32)
    for r, (v, t) in enumerate(zip(node_ids, times)):
        nbr = find_neighbors_before(adj, int(v), t)[0][-G:]
        m = len(nbr)
        rows = node_feat[nbr] if m else node_feat[:1]
        # float64 accumulation: a sequential float32 sum over 2000 rows that do not cancel is itself 2e-5 off on the G-scaled quantity
        out[r] = ((rows.astype(np.float64) * np.float64(np.float32(1.0 / max(m, 1)))).sum(axis=0) / G).astype(np.float32)
    return out


def output(P: Dict[str, torch.Tensor], link_part: torch.Tensor, node_part: torch.Tensor) -> torch.Tensor:
    return F.linear(torch.cat([link_part, node_part], dim=1), P["output_layer.weight"], P["output_layer.bias"])


def graphmixer_forward(params: Dict[str, np.ndarray], node_feat: np.ndarray, edge_feat: np.ndarray, adj: OracleAdjacency, node_ids: np.ndarray,
                       times: np.ndarray, K: int, G: int, num_layers: int, taps: bool = False, dense_node_term: bool = False):
    """compute_node_temporal_embeddings -> float32 [n, Fn] (numpy); with taps also dict(projection, layer_out, token_mean, node_term)."""
    assert K > 0 and G > 0
    node_ids = np.asarray(node_ids, dtype=np.int64)
    times = np.asarray(times, dtype=np.float64)
    P = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for k, v in params.items()}
    nf, ef = torch.from_numpy(np.ascontiguousarray(node_feat, dtype=np.float32)), torch.from_numpy(np.ascontiguousarray(edge_feat, dtype=np.float32))
    nbr, eid, ts = get_historical_neighbors_recent(adj, node_ids, times, K)
    dt = torch.from_numpy((times[:, None] - ts).astype(np.float32))              # float64 - float32 -> float64 -> .float()
    tp = {} if taps else None
    with torch.no_grad():
        link = link_encoder(P, ef, torch.from_numpy(nbr), torch.from_numpy(eid), dt, num_layers, tp)
        if dense_node_term:
            term = node_term_dense(nf, torch.from_numpy(get_historical_neighbors_recent(adj, node_ids, times, G)[0]))
        else:
            term = torch.from_numpy(node_term_rows(nf.numpy(), adj, node_ids, times, G))
        emb = output(P, link, term + nf[torch.from_numpy(node_ids)]).numpy()
    if not taps:
        return emb
    return emb, dict(projection=tp["projection"].numpy(), layer_out=[x.numpy() for x in tp["layer_out"]], token_mean=tp["token_mean"].numpy(),
                     node_term=term.numpy())
