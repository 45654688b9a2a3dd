"""Differentiable restatement of the GraphMixer TRAIN-mode forward (models/GraphMixer.py:70-150, MLPMixer :217-244, FeedForwardNet
:163-191): the operations of tests/graphmixer_oracle.py with autograd on and the four dropout sites of a Mixer block as multipliers from
oracle.dropout.Drop.mask(site, idx), indexed as dyglib_amd/csrc/graphmixer_train.hip documents (q = the root's index in the call):

    site = 4 layer + s
    s = 0: token hidden after GELU,   dense [n, C, Kh]: element (q C + ch) Kh + i
    s = 1: token FFN output,          dense [n, C, K]:  element (q C + ch) K + j
    s = 2: channel hidden after GELU, dense [n, K, H]:  element (q K + j) H + h
    s = 3: channel FFN output,        dense [n, K, C]:  element (q K + j) C + c

With drop = None it IS graphmixer_oracle.link_encoder (the eval-mode forward); drop = a float p draws the masks from torch's generator
instead (plain PyTorch dropout).  Test infrastructure: pinned to the reference's own gradients by tests/test_graphmixer_grads_cpu.py; the
GPU tests and tools/bench_graphmixer_train.py run the same operations (the latter on `cuda`); the product never imports it."""
from __future__ import annotations

from typing import Dict, Optional, Union

import numpy as np
import torch
import torch.nn.functional as F

from oracle.dropout import Drop
from oracle.dygformer_oracle import OracleAdjacency, get_historical_neighbors_recent
from tests import graphmixer_oracle as gmo


def _mask(drop, site: int, q: torch.Tensor, shape, like: torch.Tensor) -> torch.Tensor:
    """The multipliers of a [n, *shape] activation whose rows belong to the roots q [n]: element index q * prod(shape) + offset."""
    if isinstance(drop, float):          # plain PyTorch dropout (tools/bench_graphmixer_train.py): masks from torch's generator on the activation's device
        return torch.empty((len(q),) + tuple(shape), device=like.device).bernoulli_(1.0 - drop) / (1.0 - drop)
    per = int(np.prod(shape))
    idx = q.cpu().numpy().astype(np.int64).reshape(-1, 1) * per + np.arange(per, dtype=np.int64).reshape(1, -1)
    return torch.from_numpy(drop.mask(site, idx).reshape((len(q),) + tuple(shape))).to(like.device)


def link_encoder(P: Dict[str, torch.Tensor], edge_feat: torch.Tensor, nbr: torch.Tensor, eid: torch.Tensor, dt: torch.Tensor, num_layers: int,
                 drop: Union[None, float, Drop] = None, q: Optional[torch.Tensor] = None) -> torch.Tensor:
    """graphmixer_oracle.link_encoder with the four dropout sites of every block; q [n] = the roots' indices in the call (default 0 .. n-1)."""
    if drop is None:
        return gmo.link_encoder(P, edge_feat, nbr, eid, dt, num_layers)
    n = nbr.shape[0]
    q = torch.arange(n, dtype=torch.int64) if q is None else q
    tf = torch.cos((dt.double().unsqueeze(-1) * P["time_encoder.w.weight"].reshape(1, 1, -1).double() + P["time_encoder.w.bias"].double()).float())
    tf = tf.masked_fill((nbr == 0).unsqueeze(-1), 0.0)
    x = F.linear(torch.cat([edge_feat[eid], tf], dim=-1), P["projection_layer.weight"], P["projection_layer.bias"])
    for l in range(num_layers):
        p = f"mlp_mixers.{l}."
        K, Cc = x.shape[1], x.shape[2]
        h = F.layer_norm(x.permute(0, 2, 1), (K,), P[p + "token_norm.weight"], P[p + "token_norm.bias"], 1e-5)
        h = F.gelu(F.linear(h, P[p + "token_feedforward.ffn.0.weight"], P[p + "token_feedforward.ffn.0.bias"]))
        h = h * _mask(drop, 4 * l, q, (Cc, h.shape[2]), h)
        h = F.linear(h, P[p + "token_feedforward.ffn.3.weight"], P[p + "token_feedforward.ffn.3.bias"])
        h = h * _mask(drop, 4 * l + 1, q, (Cc, K), h)
        x = h.permute(0, 2, 1) + x
        h = F.layer_norm(x, (Cc,), P[p + "channel_norm.weight"], P[p + "channel_norm.bias"], 1e-5)
        h = F.gelu(F.linear(h, P[p + "channel_feedforward.ffn.0.weight"], P[p + "channel_feedforward.ffn.0.bias"]))
        h = h * _mask(drop, 4 * l + 2, q, (K, h.shape[2]), h)
        h = F.linear(h, P[p + "channel_feedforward.ffn.3.weight"], P[p + "channel_feedforward.ffn.3.bias"])
        x = h * _mask(drop, 4 * l + 3, q, (K, Cc), h) + x
    return x.mean(dim=1)


def graphmixer_train_forward(P: Dict[str, torch.Tensor], node_feat: np.ndarray, edge_feat: np.ndarray, adj: OracleAdjacency, node_ids: np.ndarray,
                             times: np.ndarray, K: int, G: int, num_layers: int, dropout_p: float = 0.0, seed: int = 0,
                             q: Optional[np.ndarray] = None) -> torch.Tensor:
    """compute_node_temporal_embeddings in train mode on the roots (node_ids, times) -> [n, Fn] with a graph.  P: parameter tensors
    (requires_grad as the caller wishes, on the CPU); the node encoder has no parameters and is taken from graphmixer_oracle.node_term_rows."""
    node_ids = np.asarray(node_ids, dtype=np.int64)
    times = np.asarray(times, dtype=np.float64)
    nf = torch.from_numpy(np.ascontiguousarray(node_feat, dtype=np.float32))
    ef = torch.from_numpy(np.ascontiguousarray(edge_feat, dtype=np.float32))
    nbr, eid, ts = get_historical_neighbors_recent(adj, node_ids, times, K)
    dt = torch.from_numpy((times[:, None] - ts).astype(np.float32))
    drop = Drop(dropout_p, seed) if dropout_p > 0 else None
    link = link_encoder(P, ef, torch.from_numpy(nbr), torch.from_numpy(eid), dt, num_layers, drop, None if q is None else torch.from_numpy(np.asarray(q, dtype=np.int64)))
    term = torch.from_numpy(gmo.node_term_rows(nf.numpy(), adj, node_ids, times, G))
    return gmo.output(P, link, term + nf[torch.from_numpy(node_ids)])
