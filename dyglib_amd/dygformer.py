"""Drop-in for the reference `DyGFormer` backbone (models/DyGFormer.py:11-317): same constructor,
same `compute_src_dst_node_temporal_embeddings` / `set_neighbor_sampler` signatures, same
parameter names and shapes (so `state_dict` round-trips with reference checkpoints) — but the whole
forward (neighbour windows, co-occurrence counts, feature gathers, time encoding, patch
projection, both encoder layers, pooling, output layer) runs inside libdygnn_hip.so with no host
round trip: the reference's numpy hop (sampling/padding/counting on the host CPU,
models/DyGFormer.py:78-106) disappears and ids never leave the GPU.

Inference (eval mode, or no_grad) runs the fused kernel.  In training mode — or whenever autograd is
recording in eval mode — the call goes through `_TrainFunction`: the training forward of
dygformer_train.hip (dropout from a counter-based generator, activations kept in a per-call
workspace) and its hand-written backward pass, so `loss.backward()` / `optimizer.step()` of
train_link_prediction.py:229-257 work unchanged.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
from torch.nn import MultiheadAttention

from . import _capi, _glue
from ._dygformer_caches import PackedWeights, ProjectedTables
from .modules import TimeEncoder
from .neighbor_sampler import NeighborSampler


class NeighborCooccurrenceEncoder(nn.Module):
    """Parameters of models/DyGFormer.py:320-335 (Linear(1,C) -> ReLU -> Linear(C,C))."""

    def __init__(self, neighbor_co_occurrence_feat_dim: int, device: str = "cpu"):
        super().__init__()
        self.neighbor_co_occurrence_feat_dim = neighbor_co_occurrence_feat_dim
        self.device = device
        self.neighbor_co_occurrence_encode_layer = nn.Sequential(
            nn.Linear(in_features=1, out_features=neighbor_co_occurrence_feat_dim),
            nn.ReLU(),
            nn.Linear(in_features=neighbor_co_occurrence_feat_dim, out_features=neighbor_co_occurrence_feat_dim))


class TransformerEncoder(nn.Module):
    """Parameters of models/DyGFormer.py:418-440 (pre-LN encoder layer)."""

    def __init__(self, attention_dim: int, num_heads: int, dropout: float = 0.1):
        super().__init__()
        self.multi_head_attention = MultiheadAttention(embed_dim=attention_dim, num_heads=num_heads, dropout=dropout)
        self.dropout = nn.Dropout(dropout)
        self.linear_layers = nn.ModuleList([nn.Linear(attention_dim, 4 * attention_dim), nn.Linear(4 * attention_dim, attention_dim)])
        self.norm_layers = nn.ModuleList([nn.LayerNorm(attention_dim), nn.LayerNorm(attention_dim)])


class _TrainFunction(torch.autograd.Function):
    """compute_src_dst_node_temporal_embeddings with gradients: forward = dygnn_dygformer_train_forward, backward =
    dygnn_dygformer_backward.  The parameters are passed as inputs only so that autograd routes their gradients."""

    @staticmethod
    def forward(ctx, model, src, dst, tms, dropout_p, seed, seq_lens, *params):
        dev = src.device
        B = src.numel()
        lib, cfg = model._lib, model._cfg
        # the fused training forward reads the kernel-ready weight copy (refreshed here after an optimizer step, launches only)
        weights, packed = model._packed_weights(dev, training=True)
        nbytes = lib.dygnn_dygformer_train_workspace_bytes(C.byref(cfg), B)
        if nbytes == 0:
            _capi.check(-3)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)          # lives until this call's backward
        out_src = torch.empty((B, model.node_feat_dim), dtype=torch.float32, device=dev)
        out_dst = torch.empty_like(out_src)
        seq = (C.c_int32 * 2)()
        if seq_lens is not None:
            seq[0], seq[1] = int(seq_lens[0]), int(seq_lens[1])
        csr = model.neighbor_sampler.csr.on_device(dev)
        rc = lib.dygnn_dygformer_train_forward(C.byref(cfg), C.byref(weights), csr, model.node_raw_features.data_ptr(),
                                               model.edge_raw_features.data_ptr(), src.data_ptr(), dst.data_ptr(), tms.data_ptr(), B,
                                               float(dropout_p), int(seed), out_src.data_ptr(), out_dst.data_ptr(), ws.data_ptr(), nbytes,
                                               C.cast(seq, C.c_void_p), packed.data_ptr(), _capi.current_stream_ptr())
        _capi.check(rc)
        ctx.model, ctx.ws, ctx.seq, ctx.B, ctx.dropout_p, ctx.seed = model, ws, seq, B, float(dropout_p), int(seed)
        ctx.packed, ctx.weights = packed, weights
        ctx.param_versions = _glue.param_versions(model._param_list())
        return out_src, out_dst

    @staticmethod
    def backward(ctx, g_src, g_dst):
        model = ctx.model
        dev = ctx.ws.device
        g_src = _glue.grad_or_zeros(g_src, (ctx.B, model.node_feat_dim), dev)
        g_dst = _glue.grad_or_zeros(g_dst, (ctx.B, model.node_feat_dim), dev)
        params = model._param_list()
        _glue.check_param_versions(params, ctx.param_versions, "DyGFormer")
        grads = _glue.zero_grads(params, dev)
        gstruct = model._weights_struct(grads)
        weights = ctx.weights
        rc = model._lib.dygnn_dygformer_backward(C.byref(model._cfg), C.byref(weights), C.byref(gstruct), g_src.data_ptr(), g_dst.data_ptr(), ctx.B,
                                                 ctx.dropout_p, ctx.seed, C.cast(ctx.seq, C.c_void_p), ctx.ws.data_ptr(), ctx.ws.numel(),
                                                 ctx.packed.data_ptr(), _capi.current_stream_ptr())
        _capi.check(rc)
        ctx.ws = None
        return (None, None, None, None, None, None, None, *grads)


class DyGFormer(nn.Module):

    def __init__(self, node_raw_features: np.ndarray, edge_raw_features: np.ndarray, neighbor_sampler: NeighborSampler,
                 time_feat_dim: int, channel_embedding_dim: int, patch_size: int = 1, num_layers: int = 2, num_heads: int = 2,
                 dropout: float = 0.1, max_input_sequence_length: int = 512, device: str = "cpu"):
        super().__init__()
        self._weights = PackedWeights()         # the kernel-ready weight copy and the projected feature tables (_dygformer_caches.py)
        self._tables = ProjectedTables()
        self._params = None                     # _param_list()
        # plain attributes, not buffers: they are not part of the state_dict (models/DyGFormer.py:32-33).  Whether a table is all zero
        # (the reference's preprocessing writes zero node features for every dataset) is established here, on the host arrays, once: the
        # fused kernel then leaves that channel out of the patch projection (table_flags of dygnn_dygformer_forward_tables)
        self._set_table("node", torch.from_numpy(np.ascontiguousarray(node_raw_features, dtype=np.float32)).to(device), not np.any(node_raw_features))
        self._set_table("edge", torch.from_numpy(np.ascontiguousarray(edge_raw_features, dtype=np.float32)).to(device), not np.any(edge_raw_features))

        self.neighbor_sampler = neighbor_sampler
        self.node_feat_dim = self.node_raw_features.shape[1]
        self.edge_feat_dim = self.edge_raw_features.shape[1]
        self.time_feat_dim = time_feat_dim
        self.channel_embedding_dim = channel_embedding_dim
        self.patch_size = patch_size
        self.num_layers = num_layers
        self.num_heads = num_heads
        self.dropout = dropout
        self.max_input_sequence_length = max_input_sequence_length
        self.device = device

        # same construction order as the reference => same default-init RNG stream per seed
        self.time_encoder = TimeEncoder(time_dim=time_feat_dim)
        self.neighbor_co_occurrence_feat_dim = self.channel_embedding_dim
        self.neighbor_co_occurrence_encoder = NeighborCooccurrenceEncoder(self.neighbor_co_occurrence_feat_dim, device=self.device)
        self.projection_layer = nn.ModuleDict({
            "node": nn.Linear(self.patch_size * self.node_feat_dim, self.channel_embedding_dim, bias=True),
            "edge": nn.Linear(self.patch_size * self.edge_feat_dim, self.channel_embedding_dim, bias=True),
            "time": nn.Linear(self.patch_size * self.time_feat_dim, self.channel_embedding_dim, bias=True),
            "neighbor_co_occurrence": nn.Linear(self.patch_size * self.neighbor_co_occurrence_feat_dim, self.channel_embedding_dim, bias=True),
        })
        self.num_channels = 4
        self.transformers = nn.ModuleList([
            TransformerEncoder(attention_dim=self.num_channels * self.channel_embedding_dim, num_heads=self.num_heads, dropout=self.dropout)
            for _ in range(self.num_layers)])
        self.output_layer = nn.Linear(self.num_channels * self.channel_embedding_dim, self.node_feat_dim, bias=True)

        self._lib = _capi.load()           # fails loudly when the HIP library is missing
        self._cfg = _capi.DygformerConfig(self.node_feat_dim, self.edge_feat_dim, self.time_feat_dim, self.channel_embedding_dim,
                                          self.patch_size, self.num_layers, self.num_heads, self.max_input_sequence_length)
        self._workspace: Dict[tuple, torch.Tensor] = {}
        self.impl = 0                      # 0 auto, 1 generic, 3 fused (see include/dygnn.h)
        # projected feature tables (_proj_plan): a table whose projected form is larger than this keeps the kernel's MFMA path
        self.proj_table_max_bytes = 1 << 30
        # constant input channels of layer 0 (_const_qkv_flag); False keeps the full product (profiles/const_qkv_ab.md has the measurements)
        self.const_qkv = True

    # ---- feature tables ------------------------------------------------------------------------
    def _set_table(self, which: str, table: torch.Tensor, all_zero: Optional[bool] = None) -> None:
        """Store a feature table with its "all zero" bit; all_zero=None looks at the tensor (one reduction, a host sync on a GPU)."""
        self.__dict__["_" + which + "_raw_features"] = table
        self.__dict__["_" + which + "_all_zero"] = bool(not table.any().item()) if all_zero is None else bool(all_zero)
        self._tables.drop()                 # the projected tables were built from the table this one replaces

    @property
    def node_raw_features(self) -> torch.Tensor:
        return self.__dict__["_node_raw_features"]

    @node_raw_features.setter
    def node_raw_features(self, table: torch.Tensor) -> None:      # a new table: its bit is established again
        self._set_table("node", table)

    @property
    def edge_raw_features(self) -> torch.Tensor:
        return self.__dict__["_edge_raw_features"]

    @edge_raw_features.setter
    def edge_raw_features(self, table: torch.Tensor) -> None:
        self._set_table("edge", table)

    @property
    def table_flags(self) -> int:
        """table_flags of dygnn_dygformer_forward_tables for the current tables.  A table edited IN PLACE after it was assigned is not
        seen: assign it again (`model.node_raw_features = model.node_raw_features`)."""
        return (_capi.TABLE_NODE_ZERO if self.__dict__["_node_all_zero"] else 0) | (_capi.TABLE_EDGE_ZERO if self.__dict__["_edge_all_zero"] else 0)

    # ---- projected feature tables --------------------------------------------------------------
    def _proj_plan(self) -> Dict[str, int]:
        """Bytes of the projected table each gathered channel gets ({} entries only for channels that get one).  The patch projection of
        the node / edge channel is linear in the gathered table rows, so W[:, slot p] . table[row] is computed once per (row, slot) and
        weights version (dygnn_dygformer_project_table) and the fused inference kernel adds patch_size rows per token instead of running
        the product.  The choice depends on the model's state only, never on a call's batch size or kernel shape: a channel gets a table
        unless its table is flagged all zero (nothing to add), `impl` pins an implementation, or the projected form exceeds
        `proj_table_max_bytes` (default 1 GiB per table; patch_size = 8 costs 2 KB per row).  Only impl = 0 — the library's own choice —
        takes the tables: impl = 1 is the generic path, and impl = 3 names the fused kernel's MFMA projection, whose bits are those of a
        plain dygnn_dygformer_forward_tables call (the split sum differs from them in the last bits).  DYGNN_PROJ_TABLES=0 (read per call)
        keeps every channel on the MFMA path, =1 builds the tables whatever their size.  The caveat of `table_flags` applies unchanged: a
        table edited IN PLACE after it was assigned is not seen — assign it again."""
        env = os.environ.get("DYGNN_PROJ_TABLES")
        plan: Dict[str, int] = {}
        if env == "0" or int(self.impl) != 0:
            return plan
        for which in ("node", "edge"):
            if self.__dict__["_" + which + "_all_zero"]:
                continue
            nbytes = int(self._lib.dygnn_dygformer_projected_bytes(C.byref(self._cfg), int(self.__dict__["_" + which + "_raw_features"].shape[0])))
            if nbytes > 0 and (env == "1" or nbytes <= int(self.proj_table_max_bytes)):
                plan[which] = nbytes
        return plan

    def _proj_flags(self, plan: Dict[str, int]) -> int:
        return (_capi.TABLE_NODE_PROJ if "node" in plan else 0) | (_capi.TABLE_EDGE_PROJ if "edge" in plan else 0)

    def _const_qkv_flag(self) -> int:
        """DYGNN_TABLE_CONST_QKV for an inference call: with the node table flagged all zero (and the edge table for the longer prefix)
        layer 0's Q/K/V products replace the k-chunks of the constant rows by one rank-3 term (include/dygnn.h).  `const_qkv =
        False` keeps the full product.  Like the projected tables it goes with the library's own choice of kernel (impl = 0): impl = 3 names the full
        product.  The library reads DYGNN_CONST_QKV=0|1 per call and lets it override this bit."""
        return _capi.TABLE_CONST_QKV if self.const_qkv and int(self.impl) == 0 and self.__dict__["_node_all_zero"] else 0

    # ---- reference API -------------------------------------------------------------------------
    def set_neighbor_sampler(self, neighbor_sampler: NeighborSampler):
        """models/DyGFormer.py:308-317."""
        _glue.reset_sampler(self, neighbor_sampler)

    def compute_src_dst_node_temporal_embeddings(self, src_node_ids, dst_node_ids, node_interact_times,
                                                 _taps: Optional[dict] = None, _group_size: int = 0, _pair_stride: int = 0
                                                 ) -> Tuple[torch.Tensor, torch.Tensor]:
        """models/DyGFormer.py:68-194.  ndarray (or already-resident device tensor) [B] int64, [B] int64,
        [B] float64 -> two float32 tensors [B, node_feat_dim] on the model's device."""
        dev = self._device()
        self._validate_ids(src_node_ids, dst_node_ids)
        src = self._to_dev(src_node_ids, torch.int64, dev)
        dst = self._to_dev(dst_node_ids, torch.int64, dev)
        tms = self._to_dev(node_interact_times, torch.float64, dev)
        B = src.numel()
        if not (dst.numel() == B and tms.numel() == B):
            raise AssertionError("src_node_ids, dst_node_ids and node_interact_times must have the same length")
        needs_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self._param_list())
        if (self.training or needs_grad) and B > 0 and _taps is None:
            if not self.training and not getattr(self, "_warned_eval_grad", False):
                # eval mode with autograd recording is a legitimate call (gradients without dropout) but ~8x slower than inference:
                # an evaluation loop that forgot torch.no_grad() should hear about it once
                import warnings
                warnings.warn("dyglib_amd.DyGFormer: eval-mode forward with autograd recording runs the training kernels (activations kept "
                              "for backward); wrap evaluation in torch.no_grad() for the fused inference kernel", RuntimeWarning, stacklevel=2)
                self._warned_eval_grad = True
            p_drop, seed = self._dropout_and_seed()
            seq_lens = self._seq_lens_groups(src_node_ids, dst_node_ids, node_interact_times, src[None], dst[None], tms[None], dev)[0]
            return _TrainFunction.apply(self, src, dst, tms, p_drop, seed, seq_lens, *self._param_list())
        out_src = torch.empty((B, self.node_feat_dim), dtype=torch.float32, device=dev)
        out_dst = torch.empty_like(out_src)
        if B == 0:
            return out_src, out_dst
        weights, packed = self._packed_weights(dev)
        ws = self._workspace_for(B, dev)
        taps_struct = None
        if _taps is not None:
            taps_struct = self._make_taps(_taps, B, dev)
        elif getattr(self, "_kernel_events", None) is not None:
            # bench.py: time the fused kernel itself (events recorded by the library around its launch), not the whole call
            e0, e1 = self._kernel_events
            taps_struct = _capi.DygformerTaps()
            taps_struct.ev_kernel_start, taps_struct.ev_kernel_stop = e0.cuda_event, e1.cuda_event
        csr = self.neighbor_sampler.csr.on_device(dev)
        proj_flags, proj_node, proj_edge = self._tables.get(self, dev, weights, self._weights.generation)
        rc = self._lib.dygnn_dygformer_forward_projected(
            C.byref(self._cfg), C.byref(weights), packed.data_ptr(), csr,
            self.node_raw_features.data_ptr(), self.edge_raw_features.data_ptr(),
            src.data_ptr(), dst.data_ptr(), tms.data_ptr(), B, int(_group_size), int(_pair_stride), out_src.data_ptr(), out_dst.data_ptr(),
            ws.data_ptr(), ws.numel(), C.byref(taps_struct) if taps_struct is not None else None,
            int(self.impl), _capi.current_stream_ptr(), self.table_flags | proj_flags | self._const_qkv_flag(),
            proj_node.data_ptr() if proj_node is not None else None, proj_edge.data_ptr() if proj_edge is not None else None)
        _capi.check(rc)
        return out_src, out_dst

    def compute_src_dst_node_temporal_embeddings_many(self, src_node_ids, dst_node_ids, node_interact_times, pos_neg_halves: bool = False):
        """Several independent reference calls in ONE launch: inputs are [N, B] (N calls of B pairs each; e.g. the
        positive and the negative call of a step, or N evaluation batches).  Row i of the result equals
        compute_src_dst_node_temporal_embeddings(src[i], dst[i], t[i]) bit for bit (every call keeps its own
        padded lengths), but the N*B pairs form one grid, which keeps all 256 CUs busy instead of B of them.
        pos_neg_halves=True (N even): calls N/2 .. N-1 are the NEGATIVE calls of calls 0 .. N/2-1 — same sources and times, other
        destinations (train_link_prediction.py:165-166) — so the kernel handles the two pairs of an edge together and gathers /
        projects the shared source side once; the rows stay bit-identical.
        Returns two float32 tensors [N, B, node_feat_dim]."""
        dev = self._device()
        self._validate_ids(src_node_ids, dst_node_ids)
        src = self._to_dev(src_node_ids, torch.int64, dev)
        dst = self._to_dev(dst_node_ids, torch.int64, dev)
        tms = self._to_dev(node_interact_times, torch.float64, dev)
        if src.dim() != 2 or src.shape != dst.shape or src.shape != tms.shape:
            raise AssertionError("expected three [N, B] arrays of equal shape")
        N, B = src.shape
        needs_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self._param_list())
        if (self.training or needs_grad) and N * B > 0:
            # training: the dense pass has ONE pair of padded lengths.  When every call of the set pads to the same lengths (the
            # usual case: some window of each call is full) the N calls are one pass over N*B pairs -- pairs never interact, so each
            # row equals the row of its own call and the parameter gradients are the sums of the per-call gradients, with half the
            # launches and no gradient-accumulation kernels; otherwise call by call.  Dropout masks are drawn per pass.
            lens = self._seq_lens_groups(src_node_ids, dst_node_ids, node_interact_times, src, dst, tms, dev)
            if all(l == lens[0] for l in lens):
                p_drop, seed = self._dropout_and_seed()
                a, b = _TrainFunction.apply(self, src.reshape(-1), dst.reshape(-1), tms.reshape(-1), p_drop, seed, lens[0], *self._param_list())
                return a.reshape(N, B, -1), b.reshape(N, B, -1)
            outs = [self.compute_src_dst_node_temporal_embeddings(src[i], dst[i], tms[i]) for i in range(N)]
            return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])
        if pos_neg_halves and N % 2 != 0:
            raise AssertionError("pos_neg_halves needs an even number of calls: [positive calls ; negative calls]")
        a, b = self.compute_src_dst_node_temporal_embeddings(src.reshape(-1), dst.reshape(-1), tms.reshape(-1), _group_size=B,
                                                             _pair_stride=(N // 2) * B if pos_neg_halves else 0)
        return a.reshape(N, B, -1), b.reshape(N, B, -1)

    def _dropout_and_seed(self):
        _glue.require_f32_params(self._param_list())
        return (float(self.dropout) if self.training else 0.0), _glue.dropout_seed(self)

    def _seq_lens_groups(self, src_in, dst_in, t_in, src: torch.Tensor, dst: torch.Tensor, tms: torch.Tensor, dev):
        """(S_src, S_dst) of each of the N calls in [N, B] device inputs (one call: [1, B] views), on the side stream: one synchronisation
        of IT, not of the main stream, so the host keeps queueing this step while the GPU still works on the previous one.  Host inputs
        (`*_in`, N * B elements each) are uploaded a second time on the side stream, ids in one copy and times in another; device inputs
        make the side stream wait for the main stream's copy of them."""
        side = getattr(self, "_side", None)
        if side is None or side.device != dev:
            side = self._side = torch.cuda.Stream(dev)
        L, P = self.max_input_sequence_length, self.patch_size
        N, B = src.shape
        host = not any(isinstance(x, torch.Tensor) for x in (src_in, dst_in, t_in))
        ev = None if host else torch.cuda.current_stream(dev).record_event()
        with torch.cuda.stream(side):
            if host:
                ids = np.stack([np.asarray(src_in, dtype=np.int64).reshape(N, B), np.asarray(dst_in, dtype=np.int64).reshape(N, B)])
                sides = torch.from_numpy(ids).to(dev)
                times = torch.from_numpy(np.ascontiguousarray(t_in, dtype=np.float64).reshape(N, B)).to(dev)
            else:
                side.wait_event(ev)
                sides, times = (src, dst), tms
            hist = torch.empty(B, dtype=torch.int32, device=dev)
            end = torch.empty(B, dtype=torch.int64, device=dev)
            maxw = torch.zeros(N, 2, dtype=torch.int32, device=dev)
            csr = self.neighbor_sampler.csr.on_device(dev)
            for i in range(N):
                for half in (0, 1):
                    _capi.check(self._lib.dygnn_window_lengths(csr, sides[half][i].data_ptr(), times[i].data_ptr(), B, L, hist.data_ptr(),
                                                               end.data_ptr(), maxw[i, half:half + 1].data_ptr(), side.cuda_stream))
            m = maxw.cpu()                               # synchronises the side stream only
        if not host:
            src.record_stream(side); dst.record_stream(side); tms.record_stream(side)
        return [tuple((int(v) + 1) + (P - (int(v) + 1) % P) % P for v in row) for row in m.tolist()]

    # ---- plumbing ------------------------------------------------------------------------------
    def _validate_ids(self, *id_arrays) -> None:
        """The reference trusts ids and fails with IndexError (list / tensor indexing); here host inputs are range-checked per call
        (two min/max over B ids) and the graph against the feature tables once per sampler, so no kernel can index outside a table."""
        n_nodes = self.node_raw_features.shape[0]
        _glue.validate_ids(self, self.neighbor_sampler.csr, id_arrays, n_nodes, n_nodes, self.edge_raw_features.shape[0])

    def invalidate_packed(self) -> None:
        """Drop the kernel-ready weight copy.  It is re-packed automatically when a parameter's version counter or address changes
        (optimizer steps, load_state_dict, .to()), on every train()/eval() switch and by this call; writes through `p.data` do not
        bump the version counter, so code that edits weights that way (custom init, EMA) calls this afterwards.  The projected feature
        tables go with it."""
        self._weights.drop()
        self._tables.drop()

    def train(self, mode: bool = True):
        self._weights.drop()
        return super().train(mode)

    def _apply(self, fn, *args, **kwargs):
        self._weights.drop()
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self._weights.drop()
        return super().load_state_dict(*args, **kwargs)

    def _device(self) -> torch.device:
        dev = self.output_layer.weight.device
        if dev.type != "cuda":
            raise _capi.DygnnError("dyglib_amd.DyGFormer runs on an MI355X only: move the model to a GPU "
                                   "(convert_to_gpu / .to('cuda')); there is no CPU fallback")
        if self.node_raw_features.device != dev:      # the reference places the tables at construction
            self._set_table("node", self.node_raw_features.to(dev), self.__dict__["_node_all_zero"])      # a copy: the bits stay
            self._set_table("edge", self.edge_raw_features.to(dev), self.__dict__["_edge_all_zero"])
        return dev

    @staticmethod
    def _to_dev(x, dtype, dev) -> torch.Tensor:
        return _glue.to_dev(x, dtype, dev, non_blocking=True)

    def _weights_struct(self, replace: Optional[list] = None) -> "_capi.DygformerWeights":
        """ctypes view of the parameters, or of `replace`: other tensors of the same shapes in the order of _param_list() (the gradient
        buffers of the backward pass)."""
        w = _capi.DygformerWeights()
        tensors = self._param_list() if replace is None else replace          # no module traversal per step
        p = lambda t: tensors[self._param_slot[id(t)]].data_ptr()
        enc = self.neighbor_co_occurrence_encoder.neighbor_co_occurrence_encode_layer
        w.time_w, w.time_b = p(self.time_encoder.w.weight), p(self.time_encoder.w.bias)
        w.cooc_w0, w.cooc_b0, w.cooc_w1, w.cooc_b1 = p(enc[0].weight), p(enc[0].bias), p(enc[2].weight), p(enc[2].bias)
        pl = self.projection_layer
        w.proj_node_w, w.proj_node_b = p(pl["node"].weight), p(pl["node"].bias)
        w.proj_edge_w, w.proj_edge_b = p(pl["edge"].weight), p(pl["edge"].bias)
        w.proj_time_w, w.proj_time_b = p(pl["time"].weight), p(pl["time"].bias)
        w.proj_cooc_w, w.proj_cooc_b = p(pl["neighbor_co_occurrence"].weight), p(pl["neighbor_co_occurrence"].bias)
        for l, tr in enumerate(self.transformers):
            L = w.layers[l]
            mha = tr.multi_head_attention
            L.in_proj_weight, L.in_proj_bias = p(mha.in_proj_weight), p(mha.in_proj_bias)
            L.out_proj_weight, L.out_proj_bias = p(mha.out_proj.weight), p(mha.out_proj.bias)
            L.ffn0_weight, L.ffn0_bias = p(tr.linear_layers[0].weight), p(tr.linear_layers[0].bias)
            L.ffn1_weight, L.ffn1_bias = p(tr.linear_layers[1].weight), p(tr.linear_layers[1].bias)
            L.norm0_weight, L.norm0_bias = p(tr.norm_layers[0].weight), p(tr.norm_layers[0].bias)
            L.norm1_weight, L.norm1_bias = p(tr.norm_layers[1].weight), p(tr.norm_layers[1].bias)
        w.output_w, w.output_b = p(self.output_layer.weight), p(self.output_layer.bias)
        return w

    def _param_list(self):
        if self._params is None:            # parameters are never added after construction
            self._params = list(self.parameters())
            self._param_slot = {id(t): i for i, t in enumerate(self._params)}
        return self._params

    def _packed_weights(self, dev, training: bool = False):
        """(ctypes view of the parameters, kernel-ready weight copy), current for this call and ordered before it on its stream."""
        return self._weights.get(self, dev, training)

    def _workspace_for(self, B: int, dev) -> torch.Tensor:
        # one workspace per (batch size, stream): calls issued on different HIP streams may overlap
        key = (B, int(self.impl), torch.cuda.current_stream(dev).cuda_stream)
        ws = self._workspace.get(key)
        if ws is None or ws.device != dev:
            nbytes = self._lib.dygnn_dygformer_workspace_bytes_for(C.byref(self._cfg), B, int(self.impl))
            ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
            if len(self._workspace) > 16:
                self._workspace.clear()
            self._workspace[key] = ws
        return ws

    def _make_taps(self, taps: dict, B: int, dev) -> "_capi.DygformerTaps":
        P, L, D = self.patch_size, self.max_input_sequence_length, self.num_channels * self.channel_embedding_dim
        t_max = 2 * ((L + P - 1) // P)
        taps["seq_lens"] = torch.zeros(2, dtype=torch.int32, device=dev)
        taps["encoder_input"] = torch.zeros((B, t_max, D), dtype=torch.float32, device=dev)
        taps["layer_outputs"] = [torch.zeros((B, t_max, D), dtype=torch.float32, device=dev) for _ in range(self.num_layers)]
        s = _capi.DygformerTaps()
        s.seq_lens = taps["seq_lens"].data_ptr()
        s.encoder_input = taps["encoder_input"].data_ptr()
        for l in range(self.num_layers):
            s.layer_out[l] = taps["layer_outputs"][l].data_ptr()
        if taps.get("want_phase_cycles"):        # only the -DDYGNN_STAMPS diagnostic build writes them
            taps["phase_cycles"] = torch.zeros((4, 8, 32), dtype=torch.int64, device=dev)
            s.phase_cycles = taps["phase_cycles"].data_ptr()
        return s
