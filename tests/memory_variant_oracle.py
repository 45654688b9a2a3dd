"""CPU restatement of the reference MemoryModel('JODIE') and MemoryModel('DyRep') forwards (models/MemoryModel.py:87-168, :267-300, :425-545) in plain torch, for the
shapes the fixtures do not cover.  The per-node Python lists of raw messages become one pending message per node: the aggregator reads only
the last element (:284-291) and lists are cleared whole (:400-407).  Imports nothing from the reference."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


class MemoryState:
    def __init__(self, num_nodes: int, memory_dim: int, message_dim: int):
        self.M = torch.zeros((num_nodes, memory_dim))
        self.U = torch.zeros(num_nodes)
        self.msg = torch.zeros((num_nodes, message_dim))
        self.msg_t = np.zeros(num_nodes, dtype=np.float64)
        self.has = np.zeros(num_nodes, dtype=bool)


def _linear1(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """nn.Linear(1, F)(x[:, None]) as the single-rounding multiply-add the reference's host addmm performs (oracle/dygformer_oracle.py
    time_encode has the story: time differences reach 1e6, where rounding the product first moves cos() visibly): the float64 product of two
    float32 is exact, so float32(float64(x) * w + b) is fma(x, w, b)."""
    return (x.double()[:, None] * w.double().reshape(1, -1) + b.double()[None, :]).float()


def _updated(params, st: MemoryState, nodes: np.ndarray):
    """get_updated_memories (:461-487) restricted to the rows that are read: nodes with a pending message take the RNNCell output and the
    message's time, the others keep what is stored"""
    M, U = st.M.clone(), st.U.clone()
    ids = np.unique(nodes[st.has[nodes]])
    if len(ids):
        i = torch.from_numpy(ids)
        p = "memory_updater.memory_updater."
        M[i] = torch.tanh(F.linear(st.msg[i], params[p + "weight_ih"], params[p + "bias_ih"]) + F.linear(st.M[i], params[p + "weight_hh"], params[p + "bias_hh"]))
        U[i] = torch.from_numpy(st.msg_t[ids]).float()
    return M, U, ids


def _commit(params, edge_feat, st: MemoryState, M, U, ids, src, dst, t, eid, other=None):
    """update_memories, clear, compute_new_node_raw_messages and store (:142-161, :212-251): source role first, then destination role; the
    last message stored for a node is the one that stays"""
    if len(ids):
        i = torch.from_numpy(ids)
        st.M[i], st.U[i] = M[i], U[i]
    st.has[np.concatenate([src, dst])] = False
    t32 = torch.from_numpy(np.asarray(t, dtype=np.float64)).float()
    w, b = params["time_encoder.w.weight"].reshape(-1), params["time_encoder.w.bias"]
    for role, (a, o) in enumerate(((src, dst), (dst, src))):
        ai, oi = torch.from_numpy(a), torch.from_numpy(o)
        dt = t32 - st.U[ai]
        # DyRep (:225-227): the other endpoint's attention embedding (other = (src rows, dst rows)) instead of its memory
        rows = torch.cat([st.M[ai], st.M[oi] if other is None else other[1 - role], torch.cos(_linear1(dt, w, b)), edge_feat[torch.from_numpy(eid)]], dim=1)
        for k in range(len(a)):
            st.msg[a[k]] = rows[k]
            st.msg_t[a[k]] = t[k]
            st.has[a[k]] = True


def jodie_forward(params, edge_feat, st: MemoryState, src, dst, t, eid, positive: bool, shifts):
    """-> (src_emb, dst_emb); params / edge_feat are torch tensors, shifts = (src mean, src std, dst mean, dst std) as Python floats"""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    M, U, ids = _updated(params, st, np.concatenate([src, dst]))
    t32 = torch.from_numpy(np.asarray(t, dtype=np.float64)).float()
    ds = (t32 - U[torch.from_numpy(src)] - shifts[0]) / shifts[1]                       # :114-118, float32 throughout
    dd = (t32 - U[torch.from_numpy(dst)] - shifts[2]) / shifts[3]
    delta = torch.cat([ds, dd])
    nodes = torch.from_numpy(np.concatenate([src, dst]))
    emb = M[nodes] * (1 + _linear1(delta, params["embedding_module.linear_layer.weight"], params["embedding_module.linear_layer.bias"]))
    if positive:
        assert eid is not None
        _commit(params, edge_feat, st, M, U, ids, src, dst, np.asarray(t, dtype=np.float64), np.asarray(eid, dtype=np.int64))
    return emb[:len(src)], emb[len(src):]


def dyrep_forward(params, node_feat, edge_feat, adj, st: MemoryState, src, dst, t, eid, positive: bool, num_layers: int, num_neighbors: int, num_heads: int = 2):
    """MemoryModel('DyRep') with `recent` sampling: returns the updated memories of the roots (:163-166); a positive call computes TGN's attention
    embedding over updated memory + raw features (oracle/tgn_oracle.py's restatement of GraphAttentionEmbedding) and stores it as the other
    endpoint's part of the new messages.  node_feat / edge_feat / params are torch tensors, adj an oracle.dygformer_oracle.OracleAdjacency."""
    from oracle import tgn_oracle as tn
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    M, U, _ = _updated(params, st, np.arange(st.M.shape[0]))                     # every node with a pending message: the attention reads neighbours
    out = M[torch.from_numpy(src)].clone(), M[torch.from_numpy(dst)].clone()
    if positive:
        assert eid is not None
        t = np.asarray(t, dtype=np.float64)
        nodes = np.concatenate([src, dst])
        emb = tn._embed(params, M + node_feat, edge_feat, adj, nodes, np.concatenate([t, t]), num_layers, num_neighbors, num_heads)
        ids = np.unique(nodes[st.has[nodes]])
        _commit(params, edge_feat, st, M, U, ids, src, dst, t, np.asarray(eid, dtype=np.int64), other=(emb[:len(src)], emb[len(src):]))
    return out
