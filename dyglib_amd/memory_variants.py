"""Drop-in for the reference `MemoryModel` with model_name == 'JODIE' (models/MemoryModel.py:9-168, :504-545): same constructor,
`compute_src_dst_node_temporal_embeddings(src_node_ids, dst_node_ids, node_interact_times, edge_ids, edges_are_positive,
num_neighbors)`, `memory_bank.__init_memory_bank__ / backup_memory_bank / reload_memory_bank / detach_memory_bank`, and the same
state_dict keys.  The nn.RNNCell memory update, the time-projection embedding and the raw-message bookkeeping run in libdygnn_hip.so
(`dygnn_jodie_forward_step`, csrc/memory_rnn.hip): inference only -- training JODIE on the HIP path is the follow-up and every call that
would need it raises.  `MemoryModel(..., model_name='JODIE')` keeps refusing; the class has its own name, like GraphMixer / TCL / CAWN.
`DyRep` below is the third arm of the reference class: TGN's modules with the RNN cell (`dygnn_dyrep_forward_step`), inference only too."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _capi, _glue
from .memory_model import GraphAttentionEmbedding, MemoryBank, MemoryModel, _init_memory_model, _memory_call_inputs
from .tgat import _tgat_weights


def compute_src_dst_node_time_shifts(src_node_ids: np.ndarray, dst_node_ids: np.ndarray, node_interact_times: np.ndarray):
    """models/MemoryModel.py:667-698: mean and (population) standard deviation of the time since a node's previous interaction in the same
    role (0 before its first), over the sources and over the destinations.  The reference walks the interactions in a Python loop; here a
    stable sort by node id puts every node's interactions next to each other in their original order, so the shifts are one subtraction.
    They are the same float64 values in the same order, hence np.mean / np.std return the reference's bits."""
    t = np.asarray(node_interact_times)

    def shifts(ids):
        ids = np.asarray(ids)
        order = np.argsort(ids, kind="stable")
        ts, sid = t[order], ids[order]
        prev = np.zeros(len(ts), dtype=ts.dtype)
        if len(ts) > 1:
            same = sid[1:] == sid[:-1]
            prev[1:][same] = ts[:-1][same]
        out = np.empty(len(ts), dtype=np.result_type(ts.dtype, np.int64) if ts.dtype.kind in "iu" else ts.dtype)
        out[order] = ts - prev
        return out

    assert len(src_node_ids) == len(dst_node_ids) == len(t)
    s, d = shifts(src_node_ids), shifts(dst_node_ids)
    return np.mean(s), np.std(s), np.mean(d), np.std(d)


class RNNMemoryUpdater(nn.Module):
    """memory_updater.memory_updater = nn.RNNCell(message_dim, memory_dim) (MemoryModel.py:504-515); the memory bank is registered under
    it too, as in the reference, so the state_dict keys coincide."""

    def __init__(self, memory_bank: MemoryBank, message_dim: int, memory_dim: int):
        super().__init__()
        self.memory_bank = memory_bank
        self.memory_updater = nn.RNNCell(input_size=message_dim, hidden_size=memory_dim)


class TimeProjectionEmbedding(nn.Module):
    """Parameters of MemoryModel.py:519-545: emb = dropout(memory * (1 + linear_layer(time interval)))."""

    def __init__(self, memory_dim: int, dropout: float):
        super().__init__()
        self.memory_dim = memory_dim
        self.dropout = nn.Dropout(dropout)
        self.linear_layer = nn.Linear(1, memory_dim)


_FOLLOW_UP = ("{name} runs inference only on the HIP path: training it there (RNNCell / time-projection backward, dropout, autograd) is a "
              "follow-up that is not built.  Call it in eval() mode under torch.no_grad()")


class JODIE(nn.Module):

    def __init__(self, node_raw_features: np.ndarray, edge_raw_features: np.ndarray, neighbor_sampler=None,
                 time_feat_dim: int = 100, model_name: str = "JODIE", num_layers: int = 2, num_heads: int = 2, dropout: float = 0.1,
                 src_node_mean_time_shift: float = 0.0, src_node_std_time_shift: float = 1.0, dst_node_mean_time_shift_dst: float = 0.0,
                 dst_node_std_time_shift: float = 1.0, device: str = "cpu"):
        super().__init__()
        if model_name != "JODIE":
            raise ValueError(f"dyglib_amd.JODIE is the reference MemoryModel with model_name 'JODIE', not {model_name!r}")
        _init_memory_model(self, node_raw_features, edge_raw_features, time_feat_dim, model_name, num_layers, num_heads, dropout, device, RNNMemoryUpdater)
        self.src_node_mean_time_shift, self.src_node_std_time_shift = src_node_mean_time_shift, src_node_std_time_shift
        self.dst_node_mean_time_shift_dst, self.dst_node_std_time_shift = dst_node_mean_time_shift_dst, dst_node_std_time_shift
        self.embedding_module = TimeProjectionEmbedding(self.memory_dim, dropout)

    def set_neighbor_sampler(self, neighbor_sampler):
        """MemoryModel.py:253-263: JODIE has no neighbours."""
        assert self.model_name in ["TGN", "DyRep"], f"Neighbor sampler is not defined in model {self.model_name}!"

    def compute_step_embeddings(self, src_node_ids, dst_node_ids, neg_src_node_ids, neg_dst_node_ids, node_interact_times, edge_ids,
                                num_neighbors: int = 20):
        """The negative call and the positive call of one batch (evaluate_models_utils.py:85-107) as ONE library call on
        [positives ; negatives]: both read the same state and only the positive call writes it, at its end.  Returns (src_emb, dst_emb,
        neg_src_emb, neg_dst_emb), bit-identical -- rows and the bank left behind -- to the negative call followed by the positive call."""
        cat = lambda a, b: (torch.cat([a, b]) if isinstance(a, torch.Tensor) else np.concatenate([np.asarray(a), np.asarray(b)]))
        n_pos = len(src_node_ids)
        s, d = self.compute_step_embeddings_joint(cat(src_node_ids, neg_src_node_ids), cat(dst_node_ids, neg_dst_node_ids),
                                                  cat(node_interact_times, node_interact_times), edge_ids, n_pos, num_neighbors)
        return s[:n_pos], d[:n_pos], s[n_pos:], d[n_pos:]

    def compute_step_embeddings_joint(self, src_pos_neg, dst_pos_neg, times_pos_neg, edge_ids, n_positive: int, num_neighbors: int = 20):
        """compute_step_embeddings for a caller that already holds the step as ONE batch [positives ; negatives] (ids and times [2B], edge
        ids [B]): returns (src_emb, dst_emb) [2B, dim] as the library wrote them."""
        return self.compute_src_dst_node_temporal_embeddings(src_pos_neg, dst_pos_neg, times_pos_neg, edge_ids, edges_are_positive=True,
                                                             num_neighbors=num_neighbors, _n_positive=int(n_positive))

    def compute_src_dst_node_temporal_embeddings(self, src_node_ids, dst_node_ids, node_interact_times, edge_ids,
                                                 edges_are_positive: bool = True, num_neighbors: int = 20, _n_positive: Optional[int] = None
                                                 ) -> Tuple[torch.Tensor, torch.Tensor]:
        """MemoryModel.py:87-168 (JODIE).  Positive calls mutate the memory bank: issue batches in chronological order.  `num_neighbors` is
        accepted and not read, as in the reference."""
        if self.training or (torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError(_FOLLOW_UP.format(name=type(self).__name__))
        dev, src, dst, tms, eids, B, n_pos = _memory_call_inputs(self, src_node_ids, dst_node_ids, node_interact_times, edge_ids, edges_are_positive, _n_positive, None)
        out = torch.empty((2, B, self.node_feat_dim), dtype=torch.float32, device=dev)      # one block: the library writes it in place
        if B == 0:
            return out[0], out[1]
        _glue.require_f32_params(self.parameters())
        cfg = _capi.TgatConfig(self.node_feat_dim, self.edge_feat_dim, self.time_feat_dim, self.num_layers, self.num_heads, int(num_neighbors))
        nbytes = self._lib.dygnn_jodie_workspace_bytes(C.byref(cfg), self.num_nodes, B)
        if nbytes == 0:
            _capi.check(-3)                      # NotImplementedError with the library's message: it names the dimension it cannot take
        ws = _glue.workspace(self._workspace, nbytes, B, 0, dev)
        cell, lin, mb = self.memory_updater.memory_updater, self.embedding_module.linear_layer, self.memory_bank
        rnn = _capi.RnnWeights(cell.weight_ih.data_ptr(), cell.weight_hh.data_ptr(), cell.bias_ih.data_ptr(), cell.bias_hh.data_ptr())
        st = _capi.TgnState(self.num_nodes, mb.node_memories.data_ptr(), mb.node_last_updated_times.data_ptr(), mb.msg.data_ptr(), mb.msg_time.data_ptr(),
                            mb.has_msg.data_ptr())
        _capi.check(self._lib.dygnn_jodie_forward_step(C.byref(cfg), self.time_encoder.w.weight.data_ptr(), self.time_encoder.w.bias.data_ptr(), C.byref(rnn),
                                                       lin.weight.data_ptr(), lin.bias.data_ptr(), float(self.src_node_mean_time_shift),
                                                       float(self.src_node_std_time_shift), float(self.dst_node_mean_time_shift_dst),
                                                       float(self.dst_node_std_time_shift), self.edge_raw_features.data_ptr(), C.byref(st), src.data_ptr(),
                                                       dst.data_ptr(), tms.data_ptr(), eids.data_ptr() if eids is not None else None, B, n_pos,
                                                       out[0].data_ptr(), out[1].data_ptr(), ws.data_ptr(), ws.numel(), _capi.current_stream_ptr()))
        return out[0], out[1]


class DyRep(MemoryModel):
    """Drop-in for the reference `MemoryModel` with model_name == 'DyRep' (models/MemoryModel.py:73-83, :125-132, :163-166, :225-227): TGN's
    modules with nn.RNNCell as the memory updater.  A call returns the updated memories of its roots; the temporal attention runs for the
    positive pairs only, where its rows enter the new raw messages (`dygnn_dyrep_forward_step` / `_levels`).  `set_neighbor_sampler`, the
    memory bank, `compute_step_embeddings` and `compute_step_embeddings_joint` are TGN's (inherited: the fused step under `recent` sampling,
    the two calls in the reference's order otherwise).  Inference only."""

    def __init__(self, node_raw_features: np.ndarray, edge_raw_features: np.ndarray, neighbor_sampler,
                 time_feat_dim: int, model_name: str = "DyRep", num_layers: int = 2, num_heads: int = 2, dropout: float = 0.1,
                 src_node_mean_time_shift: float = 0.0, src_node_std_time_shift: float = 1.0, dst_node_mean_time_shift_dst: float = 0.0,
                 dst_node_std_time_shift: float = 1.0, device: str = "cpu"):
        nn.Module.__init__(self)
        if model_name != "DyRep":
            raise ValueError(f"dyglib_amd.DyRep is the reference MemoryModel with model_name 'DyRep', not {model_name!r}")
        _init_memory_model(self, node_raw_features, edge_raw_features, time_feat_dim, model_name, num_layers, num_heads, dropout, device, RNNMemoryUpdater)
        self.src_node_mean_time_shift, self.src_node_std_time_shift = src_node_mean_time_shift, src_node_std_time_shift
        self.dst_node_mean_time_shift_dst, self.dst_node_std_time_shift = dst_node_mean_time_shift_dst, dst_node_std_time_shift
        self.embedding_module = GraphAttentionEmbedding(self.node_feat_dim, self.edge_feat_dim, self.time_feat_dim, num_layers, num_heads,
                                                        dropout, neighbor_sampler, self.time_encoder)

    def compute_src_dst_node_temporal_embeddings(self, src_node_ids, dst_node_ids, node_interact_times, edge_ids,
                                                 edges_are_positive: bool = True, num_neighbors: int = 20, _n_positive: Optional[int] = None
                                                 ) -> Tuple[torch.Tensor, torch.Tensor]:
        """MemoryModel.py:87-168 (DyRep).  Positive calls mutate the memory bank: issue batches in chronological order."""
        if self.training or (torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError(_FOLLOW_UP.format(name="DyRep"))
        sampler = self.embedding_module.neighbor_sampler
        random_strategy = sampler.sample_neighbor_strategy != "recent"
        if random_strategy and _n_positive is not None:
            raise NotImplementedError("a joint [positives ; negatives] step needs `recent` sampling (a random strategy draws per call)")
        dev, src, dst, tms, eids, B, n_pos = _memory_call_inputs(self, src_node_ids, dst_node_ids, node_interact_times, edge_ids, edges_are_positive, _n_positive,
                                                                 sampler.csr)
        out = torch.empty((2, B, self.node_feat_dim), dtype=torch.float32, device=dev)      # one block: the library writes it in place
        if B == 0:
            return out[0], out[1]
        _glue.require_f32_params(self.parameters())
        cfg = _capi.TgatConfig(self.node_feat_dim, self.edge_feat_dim, self.time_feat_dim, self.num_layers, self.num_heads, int(num_neighbors))
        em, cell = self.embedding_module, self.memory_updater.memory_updater
        w = _tgat_weights(self.time_encoder, em.temporal_conv_layers, em.merge_layers, self.num_layers)
        rnn = _capi.RnnWeights(cell.weight_ih.data_ptr(), cell.weight_hh.data_ptr(), cell.bias_ih.data_ptr(), cell.bias_hh.data_ptr())
        st = self._state()
        ws = _glue.workspace(self._workspace, self._lib.dygnn_dyrep_workspace_bytes(C.byref(cfg), self.num_nodes, B), B, num_neighbors, dev)
        tail = (self.node_raw_features.data_ptr(), self.edge_raw_features.data_ptr(), C.byref(st), src.data_ptr(), dst.data_ptr(), tms.data_ptr(),
                eids.data_ptr() if eids is not None else None, B, n_pos, out[0].data_ptr(), out[1].data_ptr(), ws.data_ptr(), ws.numel(),
                _capi.current_stream_ptr())
        if random_strategy:
            # the reference embeds [src ; dst] in every call, the negative one included, and each draw consumes the sampler's RandomState
            # (MemoryModel.py:125-132): the draws are replayed on the host in its order; a negative call throws them away, as the reference
            # throws the embedding away (:163-166)
            h = lambda x: x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
            lv, keep = self._sample_levels_host(h(src_node_ids).astype(np.int64), h(dst_node_ids).astype(np.int64), h(node_interact_times).astype(np.float64),
                                                int(num_neighbors), dev)
            _capi.check(self._lib.dygnn_dyrep_forward_levels(C.byref(cfg), C.byref(w), C.byref(rnn), C.byref(lv) if n_pos else None, *tail))
            torch.cuda.current_stream(dev).synchronize()          # `keep` (the level tensors) may be freed afterwards
            return out[0], out[1]
        _capi.check(self._lib.dygnn_dyrep_forward_step(C.byref(cfg), C.byref(w), C.byref(rnn), sampler.csr.on_device(dev), *tail))
        return out[0], out[1]
