"""Drop-in for the reference `TGAT` backbone (models/TGAT.py:9-147): same constructor, same
`compute_src_dst_node_temporal_embeddings(src_node_ids, dst_node_ids, node_interact_times, num_neighbors)` /
`compute_node_temporal_embeddings` / `set_neighbor_sampler` signatures, same parameter names (state_dict
compatible); the forward runs in libdygnn_hip.so (`dygnn_tgat_forward`, or `dygnn_tgat_forward_levels` for the random sampling
strategies, whose draws are replayed on the host).

Inference (no_grad) runs the de-duplicated level-set forward.  In training mode with autograd recording the call goes through
`_TgatTrainFunction`: the training forward of tgat_train.hip (every level entry its own row, dropout from a counter-based generator,
activations kept in a per-call workspace) and its hand-written backward pass, so `loss.backward()` / `optimizer.step()` of
train_link_prediction.py:170-185, :242-257 work unchanged.  Eval mode with autograd recording raises NotImplementedError (the result
would have no graph)."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _capi, _glue
from .modules import MergeLayer, TimeEncoder
from .neighbor_sampler import NeighborSampler


# ---- ctypes glue shared with memory_model.py (TGN runs the same library layers) ------------------------------------------------
def _tgat_weights(time_encoder, temporal_conv_layers, merge_layers, num_layers: int, replace: Optional[dict] = None) -> "_capi.TgatWeights":
    """ctypes view of the time encoder and the first `num_layers` attention / merge layers; `replace` maps id(parameter) to another tensor of
    the same shape (the gradient buffers of the backward pass)."""
    p = (lambda t: t.data_ptr()) if replace is None else (lambda t: replace[id(t)].data_ptr())
    w = _capi.TgatWeights()
    w.time_w, w.time_b = p(time_encoder.w.weight), p(time_encoder.w.bias)
    for l in range(num_layers):
        a, m, L = temporal_conv_layers[l], merge_layers[l], w.layers[l]
        L.query_w, L.key_w, L.value_w = p(a.query_projection.weight), p(a.key_projection.weight), p(a.value_projection.weight)
        L.ln_w, L.ln_b = p(a.layer_norm.weight), p(a.layer_norm.bias)
        L.res_w, L.res_b = p(a.residual_fc.weight), p(a.residual_fc.bias)
        L.fc1_w, L.fc1_b, L.fc2_w, L.fc2_b = p(m.fc1.weight), p(m.fc1.bias), p(m.fc2.weight), p(m.fc2.bias)
    return w


def _tgat_levels(ids: dict, eid: dict, dts: dict, dev):
    """Host-drawn levels ({level: array}: ids for 0..L, neighbour edge ids and time deltas for 1..L) as device tensors and their
    TgatLevels view: (struct, keep), where `keep` holds the tensors until the library's copies of them are done."""
    lv, keep = _capi.TgatLevels(), []
    for l in range(len(ids)):
        a = torch.from_numpy(np.ascontiguousarray(ids[l], dtype=np.int32)).to(dev)
        keep.append(a)
        lv.ids[l] = a.data_ptr()
        if l >= 1:
            b = torch.from_numpy(np.ascontiguousarray(eid[l], dtype=np.int32)).to(dev)
            c = torch.from_numpy(np.ascontiguousarray(dts[l], dtype=np.float32)).to(dev)
            keep += [b, c]
            lv.nbr_eid[l], lv.nbr_dt[l] = b.data_ptr(), c.data_ptr()
    return lv, keep


class _TgatTrainFunction(torch.autograd.Function):
    """compute_src_dst_node_temporal_embeddings with gradients: forward = dygnn_tgat_train_forward, backward = dygnn_tgat_backward.  The
    parameters are passed as inputs only so that autograd routes their gradients; the workspace belongs to this one call (a training step
    issues a positive and a negative call before one backward())."""

    @staticmethod
    def forward(ctx, model, src, dst, tms, num_neighbors, dropout_p, seed, levels, *params):
        dev = src.device
        B = src.numel()
        lib = model._lib
        cfg, w = model._config_and_weights(num_neighbors)
        nbytes = lib.dygnn_tgat_train_workspace_bytes(C.byref(cfg), B)
        if nbytes == 0:
            _capi.check(-3)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)          # lives until this call's backward
        out = (torch.empty((B, model.node_feat_dim), dtype=torch.float32, device=dev), torch.empty((B, model.node_feat_dim), dtype=torch.float32, device=dev))
        lv = C.byref(levels[0]) if levels is not None else None
        csr = None if levels is not None else model.neighbor_sampler.csr.on_device(dev)
        _capi.check(lib.dygnn_tgat_train_forward(C.byref(cfg), C.byref(w), csr, lv, model.node_raw_features.data_ptr(),
                                                 model.edge_raw_features.data_ptr(), src.data_ptr(), dst.data_ptr(), tms.data_ptr(), B,
                                                 float(dropout_p), int(seed), out[0].data_ptr(), out[1].data_ptr(), ws.data_ptr(), nbytes,
                                                 _capi.current_stream_ptr()))
        ctx.model, ctx.cfg, ctx.w, ctx.ws, ctx.B, ctx.dropout_p, ctx.seed = model, cfg, w, ws, B, float(dropout_p), int(seed)
        ctx.feats = (model.node_raw_features, model.edge_raw_features)        # read again by the backward pass
        ctx.levels = levels                                                    # the level tensors outlive the asynchronous copies
        ctx.param_versions = _glue.param_versions(params)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_src, g_dst):
        model = ctx.model
        dev = ctx.ws.device
        g_src = _glue.grad_or_zeros(g_src, (ctx.B, model.node_feat_dim), dev)
        g_dst = _glue.grad_or_zeros(g_dst, (ctx.B, model.node_feat_dim), dev)
        params = model._param_list()
        _glue.check_param_versions(params, ctx.param_versions, "TGAT")
        grads = _glue.zero_grads(params, dev)
        gstruct = _tgat_weights(model.time_encoder, model.temporal_conv_layers, model.merge_layers, model.num_layers,
                                {id(p): g for p, g in zip(params, grads)})
        _capi.check(model._lib.dygnn_tgat_backward(C.byref(ctx.cfg), C.byref(ctx.w), C.byref(gstruct), g_src.data_ptr(), g_dst.data_ptr(), ctx.B,
                                                   ctx.dropout_p, ctx.seed, ctx.ws.data_ptr(), ctx.ws.numel(), _capi.current_stream_ptr()))
        ctx.ws = ctx.levels = ctx.feats = None
        return (None,) * 8 + tuple(grads)


class MultiHeadAttention(nn.Module):
    """Parameters of models/modules.py:99-135 (bias-free q/k/v projections, LayerNorm, residual_fc)."""

    def __init__(self, node_feat_dim: int, edge_feat_dim: int, time_feat_dim: int, num_heads: int = 2, dropout: float = 0.1):
        super().__init__()
        self.node_feat_dim, self.edge_feat_dim, self.time_feat_dim, self.num_heads = node_feat_dim, edge_feat_dim, time_feat_dim, num_heads
        self.query_dim = node_feat_dim + time_feat_dim
        self.key_dim = node_feat_dim + edge_feat_dim + time_feat_dim
        assert self.query_dim % num_heads == 0, "The sum of node_feat_dim and time_feat_dim should be divided by num_heads!"
        self.head_dim = self.query_dim // num_heads
        self.query_projection = nn.Linear(self.query_dim, num_heads * self.head_dim, bias=False)
        self.key_projection = nn.Linear(self.key_dim, num_heads * self.head_dim, bias=False)
        self.value_projection = nn.Linear(self.key_dim, num_heads * self.head_dim, bias=False)
        self.scaling_factor = self.head_dim ** -0.5
        self.layer_norm = nn.LayerNorm(self.query_dim)
        self.residual_fc = nn.Linear(num_heads * self.head_dim, self.query_dim)
        self.dropout = nn.Dropout(dropout)


class TGAT(nn.Module):

    def __init__(self, node_raw_features: np.ndarray, edge_raw_features: np.ndarray, neighbor_sampler: NeighborSampler,
                 time_feat_dim: int, num_layers: int = 2, num_heads: int = 2, dropout: float = 0.1, device: str = "cpu"):
        super().__init__()
        self.node_raw_features = torch.from_numpy(np.ascontiguousarray(node_raw_features, dtype=np.float32)).to(device)
        self.edge_raw_features = torch.from_numpy(np.ascontiguousarray(edge_raw_features, dtype=np.float32)).to(device)
        self.neighbor_sampler = neighbor_sampler
        self.node_feat_dim = self.node_raw_features.shape[1]
        self.edge_feat_dim = self.edge_raw_features.shape[1]
        self.time_feat_dim = time_feat_dim
        self.num_layers = num_layers
        self.num_heads = num_heads
        self.dropout = dropout
        self.time_encoder = TimeEncoder(time_dim=time_feat_dim)
        self.temporal_conv_layers = nn.ModuleList([MultiHeadAttention(self.node_feat_dim, self.edge_feat_dim, self.time_feat_dim,
                                                                      self.num_heads, self.dropout) for _ in range(num_layers)])
        self.merge_layers = nn.ModuleList([MergeLayer(input_dim1=self.node_feat_dim + self.time_feat_dim, input_dim2=self.node_feat_dim,
                                                      hidden_dim=self.node_feat_dim, output_dim=self.node_feat_dim) for _ in range(num_layers)])
        self._lib = _capi.load()
        self._workspace: Dict[tuple, torch.Tensor] = {}

    def set_neighbor_sampler(self, neighbor_sampler: NeighborSampler):
        """models/TGAT.py:138-147."""
        _glue.reset_sampler(self, neighbor_sampler)

    def compute_src_dst_node_temporal_embeddings(self, src_node_ids, dst_node_ids, node_interact_times,
                                                 num_neighbors: int = 20) -> Tuple[torch.Tensor, torch.Tensor]:
        """models/TGAT.py:48-64: two float32 tensors [B, node_feat_dim] on the model's device.  With autograd recording in training
        mode the call is differentiable (_TgatTrainFunction; dropout `self.dropout`)."""
        train = torch.is_grad_enabled() and (self.training or any(p.requires_grad for p in self.parameters()))
        if train and not self.training:
            # eval mode with autograd recording would return tensors without a graph: loss.backward() would silently do nothing
            raise NotImplementedError("TGAT forward with autograd recording in eval mode is not built on the HIP path: call it under "
                                      "torch.no_grad(), or use model.train() (with model.dropout = 0.0 for dropout-free gradients)")
        random_strategy = self.neighbor_sampler.sample_neighbor_strategy != "recent"
        self.neighbor_sampler._check_strategy()
        dev = self._prepare(src_node_ids, dst_node_ids)
        src, dst = _glue.to_dev(src_node_ids, torch.int64, dev), _glue.to_dev(dst_node_ids, torch.int64, dev)
        tms = _glue.to_dev(node_interact_times, torch.float64, dev)
        B = src.numel()
        assert dst.numel() == B and tms.numel() == B
        if train and B > 0:
            p_drop, seed = self._dropout_and_seed()
            levels = None
            if random_strategy:       # the RandomState is consumed exactly as by an inference call
                levels = self._sample_levels_host(src.cpu().numpy(), dst.cpu().numpy(), tms.cpu().numpy(), int(num_neighbors), dev)
            return _TgatTrainFunction.apply(self, src, dst, tms, int(num_neighbors), p_drop, seed, levels, *self._param_list())
        out = torch.empty((2, B, self.node_feat_dim), dtype=torch.float32, device=dev)      # one block: the library writes it in place
        out_src, out_dst = out[0], out[1]
        if B == 0:
            return out_src, out_dst
        cfg, w = self._config_and_weights(num_neighbors)
        ws = _glue.workspace(self._workspace, self._lib.dygnn_tgat_workspace_bytes(C.byref(cfg), B), B, num_neighbors, dev)
        if random_strategy:
            lv, keep = self._sample_levels_host(src.cpu().numpy(), dst.cpu().numpy(), tms.cpu().numpy(), int(num_neighbors), dev)
            _capi.check(self._lib.dygnn_tgat_forward_levels(C.byref(cfg), C.byref(w), C.byref(lv), self.node_raw_features.data_ptr(),
                                                            self.edge_raw_features.data_ptr(), B, out_src.data_ptr(), out_dst.data_ptr(),
                                                            ws.data_ptr(), ws.numel(), _capi.current_stream_ptr()))
            torch.cuda.current_stream(dev).synchronize()          # `keep` (the level tensors) may be freed afterwards
            return out_src, out_dst
        self._last_call = (cfg, B, ws)
        _capi.check(self._lib.dygnn_tgat_forward(C.byref(cfg), C.byref(w), self.neighbor_sampler.csr.on_device(dev),
                                                 self.node_raw_features.data_ptr(), self.edge_raw_features.data_ptr(),
                                                 src.data_ptr(), dst.data_ptr(), tms.data_ptr(), B, out_src.data_ptr(), out_dst.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), _capi.current_stream_ptr()))
        return out_src, out_dst

    def compute_step_embeddings(self, src_node_ids, dst_node_ids, neg_dst_node_ids, node_interact_times, num_neighbors: int = 20):
        """The positive and the negative call of an evaluation step (evaluate_models_utils.py:126-136) as ONE library call on the roots
        [sources ; destinations ; negative destinations] at the batch times (dygnn_tgat_forward_roots): the negative call's sources are the
        positive call's (:62-63) and a root's row does not depend on the batch it is in, so (src_emb, dst_emb, neg_dst_emb) are bit-identical to
        compute_src_dst_node_temporal_embeddings(src, dst, t) and (src, neg_dst, t)[1].  `recent` sampling only (the random strategies consume the
        sampler's RandomState call by call)."""
        if self.neighbor_sampler.sample_neighbor_strategy != "recent":
            raise NotImplementedError("compute_step_embeddings: `recent` sampling only; issue the two calls of the reference for the random strategies")
        if torch.is_grad_enabled() and (self.training or any(p.requires_grad for p in self.parameters())):
            # inference only: sharing the source rows would share their dropout masks, which the reference's two training calls do not
            raise NotImplementedError("compute_step_embeddings is inference-only: call it under torch.no_grad(), or issue the two "
                                      "compute_src_dst_node_temporal_embeddings calls of the reference for training")
        dev = self._prepare(src_node_ids, dst_node_ids, neg_dst_node_ids)
        parts_i = [_glue.to_dev(ids, torch.int64, dev) for ids in (src_node_ids, dst_node_ids, neg_dst_node_ids)]
        tms = _glue.to_dev(node_interact_times, torch.float64, dev)
        B = parts_i[0].numel()
        assert parts_i[1].numel() == B and parts_i[2].numel() == B and tms.numel() == B
        pad = (3 * B) % 2                                   # the library takes an even number of roots: repeat the last one
        roots = torch.cat(parts_i + ([parts_i[2][-1:]] if pad and B else []))
        times = torch.cat([tms, tms, tms] + ([tms[-1:]] if pad and B else []))
        n = roots.numel()
        out = torch.empty((n, self.node_feat_dim), dtype=torch.float32, device=dev)
        if B == 0:
            return out[:0], out[:0], out[:0]
        cfg, w = self._config_and_weights(num_neighbors)
        ws = _glue.workspace(self._workspace, self._lib.dygnn_tgat_workspace_bytes(C.byref(cfg), n // 2), n // 2, num_neighbors, dev)
        self._last_call = (cfg, n // 2, ws)
        _capi.check(self._lib.dygnn_tgat_forward_roots(C.byref(cfg), C.byref(w), self.neighbor_sampler.csr.on_device(dev), self.node_raw_features.data_ptr(),
                                                       self.edge_raw_features.data_ptr(), roots.data_ptr(), times.data_ptr(), n, out.data_ptr(),
                                                       ws.data_ptr(), ws.numel(), _capi.current_stream_ptr()))
        return out[:B], out[B:2 * B], out[2 * B:3 * B]

    def _prepare(self, *id_arrays):
        """What both entry points do first: refuse a non-cuda model, move the feature tables to its device, check the tables against the
        sampler's graph (once per sampler: every id reachable through it is inside them) and the query ids against the node table
        (IndexError like the reference, models/TGAT.py:85).  Returns the device."""
        dev = self.merge_layers[0].fc1.weight.device
        _glue.require_cuda_tables(self, dev)
        n_nodes = self.node_raw_features.shape[0]
        _glue.validate_ids(self, self.neighbor_sampler.csr, id_arrays, n_nodes, n_nodes, self.edge_raw_features.shape[0])
        return dev

    def _config_and_weights(self, num_neighbors: int):
        cfg = _capi.TgatConfig(self.node_feat_dim, self.edge_feat_dim, self.time_feat_dim, self.num_layers, self.num_heads, int(num_neighbors))
        return cfg, _tgat_weights(self.time_encoder, self.temporal_conv_layers, self.merge_layers, self.num_layers)

    def _param_list(self):
        return list(self.parameters())

    def _dropout_and_seed(self):
        _glue.require_f32_params(self._param_list())
        return (float(self.dropout) if self.training else 0.0), _glue.dropout_seed(self)

    def compute_node_temporal_embeddings(self, node_ids, node_interact_times, current_layer_num: int, num_neighbors: int = 20) -> torch.Tensor:
        """models/TGAT.py:66-136: the embedding of `node_ids` at `node_interact_times` after `current_layer_num` layers ([n, node_feat_dim]).
        Layer 0 is the raw node feature row (:85-88); layer l is the l-layer model over the first l conv / merge layers (the recursion only
        ever descends, :92-110), i.e. one library call with num_layers = l on the nodes as both sides (`recent`: duplicates are computed once)."""
        assert current_layer_num >= 0                                                      # models/TGAT.py:77
        if current_layer_num > self.num_layers:
            raise IndexError("index out of range in temporal_conv_layers")              # ModuleList indexing in the reference (:123)
        if current_layer_num == 0:
            self.neighbor_sampler.csr.check_query_ids(node_ids, limit=self.node_raw_features.shape[0])
            idx = node_ids if isinstance(node_ids, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(node_ids, dtype=np.int64))
            return self.node_raw_features[idx.to(self.node_raw_features.device)]
        full = self.num_layers
        try:
            self.num_layers = int(current_layer_num)
            emb, _ = self.compute_src_dst_node_temporal_embeddings(node_ids, node_ids, node_interact_times, num_neighbors=num_neighbors)
        finally:
            self.num_layers = full
        return emb

    def last_level_entries(self) -> Tuple[int, int]:
        """(entries over the computed levels, entries actually computed) of the last `recent` call: two-layer models compute every
        distinct (node, time) entry of level 1 once (dygnn_tgat_level_entries; synchronises the stream)."""
        cfg, B, ws = self._last_call
        total, computed = C.c_int64(0), C.c_int64(0)
        _capi.check(self._lib.dygnn_tgat_level_entries(C.byref(cfg), B, ws.data_ptr(), C.byref(total), C.byref(computed), _capi.current_stream_ptr()))
        return int(total.value), int(computed.value)

    # ---- random sampling strategies: the draws are replayed on the host in the reference's recursion order ----------------
    def _sample_levels_host(self, src: np.ndarray, dst: np.ndarray, t: np.ndarray, k: int, dev):
        """Level sets for dygnn_tgat_forward_levels.  models/TGAT.py:92-110: compute_node_temporal_embeddings(nodes, l) first
        recurses for the nodes themselves at layer l-1 (drawing THEIR neighbours), then draws the layer-l neighbours, then
        recurses for those; src is processed completely before dst (models/TGAT.py:57-62).  With a random sampler every one of
        those draws is independent and must consume the RandomState in exactly that order."""
        if self.num_layers not in (1, 2):
            raise NotImplementedError("TGAT with a random sampling strategy is built for num_layers 1 and 2")
        smp = self.neighbor_sampler
        L = self.num_layers

        def draw(nodes, times):
            n, e, tn = smp.get_historical_neighbors(nodes, times, num_neighbors=k)            # host round trip, RandomState replay
            dt = (times[:, None] - tn).astype(np.float32)                                     # models/TGAT.py:116-119
            return n, e, tn, dt

        per_side = []
        for nodes in (src, dst):
            if L == 1:
                per_side.append({"top": draw(nodes, t)})
            else:
                d1 = draw(nodes, t)                                        # neighbours of the nodes themselves, for their layer-1 embedding
                d2 = draw(nodes, t)                                        # layer-2 neighbours
                d3 = draw(d2[0].reshape(-1), d2[2].reshape(-1).astype(np.float64))           # neighbours of those, for THEIR layer-1 embedding
                per_side.append({"self": d1, "top": d2, "nbr": d3})
        s_, d_ = per_side
        ids = {L: np.concatenate([src, dst])}
        eid, dts = {}, {}
        eid[L] = np.concatenate([s_["top"][1], d_["top"][1]])
        dts[L] = np.concatenate([s_["top"][3], d_["top"][3]])
        ids[L - 1] = np.concatenate([ids[L], s_["top"][0].reshape(-1), d_["top"][0].reshape(-1)])
        if L == 2:
            eid[1] = np.concatenate([s_["self"][1], d_["self"][1], s_["nbr"][1], d_["nbr"][1]])
            dts[1] = np.concatenate([s_["self"][3], d_["self"][3], s_["nbr"][3], d_["nbr"][3]])
            nb1 = np.concatenate([s_["self"][0], d_["self"][0], s_["nbr"][0], d_["nbr"][0]])
            ids[0] = np.concatenate([ids[1], nb1.reshape(-1)])
        return _tgat_levels(ids, eid, dts, dev)
