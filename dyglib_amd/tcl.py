"""Drop-in for the reference `TCL` backbone (models/TCL.py:9-188): same constructor, same
`compute_src_dst_node_temporal_embeddings(src_node_ids, dst_node_ids, node_interact_times, num_neighbors)` / `set_neighbor_sampler`
signatures, same parameter names and shapes (a reference checkpoint loads with strict=True); the forward runs in libdygnn_hip.so
(`dygnn_tcl_forward`, dyglib_amd/csrc/tcl.hip).

Inference (eval or train mode under torch.no_grad()) takes `dygnn_tcl_forward`.  Training (train mode with autograd recording) takes
`dygnn_tcl_train_forward` / `dygnn_tcl_backward` (dyglib_amd/csrc/tcl_train.hip) through `_TclTrainFunction`: dropout `self.dropout` from the
counter-based generator of dropout.h, every parameter receives a gradient, the feature tables do not.  Eval mode with autograd recording, and
`compute_step_embeddings` (the evaluation step) with autograd recording in either mode, raise NotImplementedError.  All three neighbour
sampling strategies work: the neighbours are sampled by `NeighborSampler.get_historical_neighbors_device` in the reference's call order
(sources, then destinations) and handed to the library, on both paths.

In TCL the source embedding depends on the destination it is paired with (cross-attention), so an evaluation step has FOUR results:
`compute_step_embeddings` returns (src of the positive call, dst, src of the negative call, neg_dst)."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _capi, _glue
from .modules import TimeEncoder, TransformerEncoder, fill_encoder_layer_weights
from .neighbor_sampler import NeighborSampler


class _TclTrainFunction(torch.autograd.Function):
    """compute_src_dst_node_temporal_embeddings with gradients: forward = dygnn_tcl_train_forward, backward = dygnn_tcl_backward.  The
    parameters are passed as inputs only so that autograd routes their gradients; the workspace belongs to this one call (a training step
    issues a negative and a positive call before one backward())."""

    @staticmethod
    def forward(ctx, model, sides, B, num_neighbors, dropout_p, seed, *params):
        dev = model.output_layer.weight.device
        d = model.node_feat_dim
        out = (torch.empty((B, d), dtype=torch.float32, device=dev), torch.empty((B, d), dtype=torch.float32, device=dev))
        ctx.model, ctx.B = model, B
        if B == 0:                                                           # nothing to launch, here or in backward
            return out
        lib = model._lib
        cfg, w = model._config(num_neighbors), model._weights()
        nbytes = lib.dygnn_tcl_train_workspace_bytes(C.byref(cfg), B)
        if nbytes == 0:                                  # AssertionError (bad argument) or NotImplementedError (unsupported) with the library's message
            _capi.check(lib.dygnn_tcl_check(C.byref(cfg)))
            _capi.check(-1)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)          # lives until this call's backward
        roots, tms, nbr, eid, nts = sides
        _capi.check(lib.dygnn_tcl_train_forward(C.byref(cfg), C.byref(w), model.node_raw_features.data_ptr(), model.edge_raw_features.data_ptr(),
                                                roots.data_ptr(), tms.data_ptr(), nbr.data_ptr(), eid.data_ptr(), nts.data_ptr(), B, float(dropout_p),
                                                int(seed), out[0].data_ptr(), out[1].data_ptr(), ws.data_ptr(), nbytes, _capi.current_stream_ptr()))
        ctx.cfg, ctx.w, ctx.ws, ctx.dropout_p, ctx.seed = cfg, w, ws, float(dropout_p), int(seed)
        ctx.feats = (model.node_raw_features, model.edge_raw_features)        # regathered by the backward pass
        ctx.param_versions = _glue.param_versions(params)
        return out

    @staticmethod
    def backward(ctx, g_src, g_dst):
        model = ctx.model
        params = list(model.parameters())
        if ctx.B == 0:
            return (None,) * (6 + len(params))
        dev = ctx.ws.device
        g_src = _glue.grad_or_zeros(g_src, (ctx.B, model.node_feat_dim), dev)
        g_dst = _glue.grad_or_zeros(g_dst, (ctx.B, model.node_feat_dim), dev)
        _glue.check_param_versions(params, ctx.param_versions, "TCL")
        grads = _glue.zero_grads(params, dev)
        gstruct = model._weights({id(p): g for p, g in zip(params, grads)})
        _capi.check(model._lib.dygnn_tcl_backward(C.byref(ctx.cfg), C.byref(ctx.w), C.byref(gstruct), g_src.data_ptr(), g_dst.data_ptr(), ctx.B,
                                                  ctx.dropout_p, ctx.seed, ctx.ws.data_ptr(), ctx.ws.numel(), _capi.current_stream_ptr()))
        ctx.ws = ctx.feats = None
        return (None,) * 6 + tuple(grads)


class TCL(nn.Module):

    def __init__(self, node_raw_features: np.ndarray, edge_raw_features: np.ndarray, neighbor_sampler: NeighborSampler,
                 time_feat_dim: int, num_layers: int = 2, num_heads: int = 2, num_depths: int = 20, dropout: float = 0.1, device: str = "cpu"):
        super().__init__()
        self.node_raw_features = torch.from_numpy(np.ascontiguousarray(node_raw_features, dtype=np.float32)).to(device)
        self.edge_raw_features = torch.from_numpy(np.ascontiguousarray(edge_raw_features, dtype=np.float32)).to(device)
        self.neighbor_sampler = neighbor_sampler
        self.node_feat_dim = self.node_raw_features.shape[1]
        self.edge_feat_dim = self.edge_raw_features.shape[1]
        self.time_feat_dim = time_feat_dim
        self.num_layers = num_layers
        self.num_heads = num_heads
        self.num_depths = num_depths
        self.dropout = dropout
        self.device = device
        self.time_encoder = TimeEncoder(time_dim=time_feat_dim)
        self.depth_embedding = nn.Embedding(num_embeddings=num_depths, embedding_dim=self.node_feat_dim)
        self.projection_layer = nn.ModuleDict({
            "node": nn.Linear(self.node_feat_dim, self.node_feat_dim, bias=True),
            "edge": nn.Linear(self.edge_feat_dim, self.node_feat_dim, bias=True),
            "time": nn.Linear(self.time_feat_dim, self.node_feat_dim, bias=True)})
        self.transformers = nn.ModuleList([TransformerEncoder(self.node_feat_dim, self.num_heads, self.dropout) for _ in range(self.num_layers)])
        self.output_layer = nn.Linear(self.node_feat_dim, self.node_feat_dim, bias=True)
        self._lib = _capi.load()
        self._workspace: Dict[tuple, torch.Tensor] = {}

    def set_neighbor_sampler(self, neighbor_sampler: NeighborSampler):
        """models/TCL.py:179-188."""
        _glue.reset_sampler(self, neighbor_sampler)

    # ---- the reference's entry point ---------------------------------------------------------------------------------------------------
    def compute_src_dst_node_temporal_embeddings(self, src_node_ids, dst_node_ids, node_interact_times, num_neighbors: int = 20,
                                                 taps: Optional[int] = None):
        """models/TCL.py:56-154: two float32 tensors [B, node_feat_dim]; ONE library call on the sides [src ; dst] and the pairs (i, B + i).
        `taps` = r (not in the reference): also return the intermediates of the first r pairs, (src, dst, dict(encoder_input [r, 2, S, d],
        layer_out: per layer [r, 2, S, d])); index 0 / 1 of the second axis is the source / destination sequence.
        In train mode with autograd recording the call is differentiable (dropout self.dropout; `taps` are refused there)."""
        train = self.training and torch.is_grad_enabled()
        (src, dst), tms = self._inputs((src_node_ids, dst_node_ids), node_interact_times, num_neighbors, trainable=True)
        B = src.numel()
        sides = self._sample([src, dst], tms, num_neighbors)
        if train:
            if taps is not None:
                raise NotImplementedError("tcl: taps are an inference facility; the training path does not return intermediates")
            if len(self.transformers) != self.num_layers or self.num_layers > _capi.DYGNN_MAX_LAYERS:
                raise NotImplementedError(f"tcl: num_layers {self.num_layers} not supported (1..{_capi.DYGNN_MAX_LAYERS})")
            return _TclTrainFunction.apply(self, sides, B, int(num_neighbors), float(self.dropout), _glue.dropout_seed(self), *self.parameters())
        idx = np.arange(B, dtype=np.int32)
        out = self._forward(*sides, idx, idx + B, num_neighbors, taps)
        return out if taps is None else (out[0], out[1], out[2])

    def compute_step_embeddings(self, src_node_ids, dst_node_ids, neg_dst_node_ids, node_interact_times, num_neighbors: int = 20
                                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """The positive and the negative call of an evaluation step (evaluate_models_utils.py:126-136) as ONE library call: (src_pos, dst,
        src_neg, neg_dst), bit-identical to compute_src_dst...(src, dst) followed by compute_src_dst...(src, neg_dst).  With `recent` sampling
        the source sides are shared between the two pairs of an edge (sides [src ; dst ; neg_dst], 2 B pairs); a random strategy samples in
        the order of the reference's two calls (src, dst, src, neg_dst), so the sources are drawn twice and are four B sides."""
        (src, dst, neg), tms = self._inputs((src_node_ids, dst_node_ids, neg_dst_node_ids), node_interact_times, num_neighbors)
        B = src.numel()
        idx = np.arange(B, dtype=np.int32)
        if self.neighbor_sampler.sample_neighbor_strategy == "recent":
            sides = self._sample([src, dst, neg], tms, num_neighbors)
            a, b = np.concatenate([idx, idx]), np.concatenate([idx + B, idx + 2 * B])
        else:
            sides = self._sample([src, dst, src, neg], tms, num_neighbors)
            a, b = np.concatenate([idx, idx + 2 * B]), np.concatenate([idx + B, idx + 3 * B])
        oa, ob = self._forward(*sides, a, b, num_neighbors)
        return oa[:B], ob[:B], oa[B:], ob[B:]

    # ---- glue ------------------------------------------------------------------------------------------------------------------------
    def _inputs(self, id_arrays, node_interact_times, num_neighbors, trainable: bool = False):
        """Refuse what is not built (autograd recording outside the training call, a CPU model), validate host ids like the reference
        (IndexError; a root id of 0 is an AssertionError: the reference returns NaN rows for it, every key being masked), and move ids (int64)
        and times (float64) to the model's device.  `trainable`: the caller has a differentiable path for train mode."""
        _glue.refuse_untrainable(self, trainable, "this TCL call is inference-only on the HIP path: call it under torch.no_grad().  Gradients flow "
                                 "through compute_src_dst_node_temporal_embeddings in train mode only (eval mode and compute_step_embeddings "
                                 "have no backward pass)")
        self.neighbor_sampler._check_strategy()
        assert num_neighbors > 0, "Number of sampled neighbors for each node should be greater than 0!"          # utils/utils.py:157
        assert num_neighbors + 1 == self.depth_embedding.weight.shape[0], \
            f"tcl: num_neighbors + 1 ({num_neighbors + 1}) must equal num_depths ({self.depth_embedding.weight.shape[0]})"      # models/TCL.py:173
        dev = self.output_layer.weight.device
        _glue.require_cuda_tables(self, dev)
        n_nodes = self.node_raw_features.shape[0]
        _glue.validate_ids(self, self.neighbor_sampler.csr, id_arrays, n_nodes, n_nodes, self.edge_raw_features.shape[0])
        for ids in id_arrays:
            if not isinstance(ids, torch.Tensor) and np.asarray(ids).size:
                assert int(np.asarray(ids).min()) > 0, "tcl: node id 0 is the padding node: as a root it has no valid attention key"
        parts = [_glue.to_dev(ids, torch.int64, dev).reshape(-1) for ids in id_arrays]
        tms = _glue.to_dev(node_interact_times, torch.float64, dev).reshape(-1)
        assert all(p.numel() == tms.numel() for p in parts)
        return parts, tms

    def _sample(self, parts, tms, num_neighbors):
        """One sampler call per part, in order (the order matters for the random strategies) -> the sides' device arrays."""
        smp = self.neighbor_sampler
        if smp.device != tms.device:
            raise _capi.DygnnError(f"the neighbor sampler is on {smp.device}, the model on {tms.device}")
        drawn = [smp.get_historical_neighbors_device(p, tms, num_neighbors) for p in parts] if tms.numel() else []
        if not drawn:
            return None, None, None, None, None
        cat = lambda xs: xs[0] if len(xs) == 1 else torch.cat(xs)
        return (cat(parts), cat([tms] * len(parts)), cat([d[0] for d in drawn]), cat([d[1] for d in drawn]), cat([d[2] for d in drawn]))

    def _config(self, num_neighbors: int) -> "_capi.TclConfig":
        return _capi.TclConfig(self.node_feat_dim, self.edge_feat_dim, self.time_feat_dim, int(num_neighbors), self.num_layers, self.num_heads,
                               self.node_raw_features.shape[0], self.edge_raw_features.shape[0])

    def _weights(self, replace: Optional[dict] = None) -> "_capi.TclWeights":
        """ctypes view of the parameters; `replace` maps id(parameter) to another tensor of the same shape (the gradient buffers of the
        backward pass)."""
        _glue.require_f32_params(self.parameters())
        w = _capi.TclWeights()
        p = (lambda t: t.data_ptr()) if replace is None else (lambda t: replace[id(t)].data_ptr())
        w.time_w, w.time_b, w.depth_w = p(self.time_encoder.w.weight), p(self.time_encoder.w.bias), p(self.depth_embedding.weight)
        pl = self.projection_layer
        w.proj_node_w, w.proj_node_b = p(pl["node"].weight), p(pl["node"].bias)
        w.proj_edge_w, w.proj_edge_b = p(pl["edge"].weight), p(pl["edge"].bias)
        w.proj_time_w, w.proj_time_b = p(pl["time"].weight), p(pl["time"].bias)
        for l, t in enumerate(self.transformers):
            fill_encoder_layer_weights(w.layers[l], t, p)
        w.output_w, w.output_b = p(self.output_layer.weight), p(self.output_layer.bias)
        return w

    def _forward(self, roots, tms, nbr, eid, nts, pair_a: np.ndarray, pair_b: np.ndarray, num_neighbors: int, taps: Optional[int] = None):
        dev = self.output_layer.weight.device
        P = len(pair_a)
        n_sides = 0 if roots is None else roots.numel()
        cfg = self._config(num_neighbors)
        if len(self.transformers) != self.num_layers or self.num_layers > _capi.DYGNN_MAX_LAYERS:
            raise NotImplementedError(f"tcl: num_layers {self.num_layers} not supported (1..{_capi.DYGNN_MAX_LAYERS})")
        nbytes = self._lib.dygnn_tcl_workspace_bytes(C.byref(cfg), n_sides, P)
        if nbytes == 0:                                  # AssertionError (bad argument) or NotImplementedError (unsupported) with the library's message
            _capi.check(self._lib.dygnn_tcl_check(C.byref(cfg)))
        ws = _glue.workspace(self._workspace, nbytes, (n_sides, P), num_neighbors, dev)
        d, S = self.node_feat_dim, int(num_neighbors) + 1
        out_a = torch.empty((P, d), dtype=torch.float32, device=dev)
        out_b = torch.empty((P, d), dtype=torch.float32, device=dev)
        tap_struct, tap_out = None, None
        if taps is not None:
            r = min(int(taps), P)
            new = lambda: torch.zeros((r, 2, S, d), dtype=torch.float32, device=dev)
            tap_out = dict(encoder_input=new(), layer_out=[new() for _ in range(self.num_layers)])
            tap_struct = _capi.TclTaps()
            tap_struct.rows = r
            tap_struct.encoder_input = tap_out["encoder_input"].data_ptr()
            for l, t in enumerate(tap_out["layer_out"]):
                tap_struct.layer_out[l] = t.data_ptr()
        if P > 0:
            pa, pb = np.ascontiguousarray(pair_a, dtype=np.int32), np.ascontiguousarray(pair_b, dtype=np.int32)
            _capi.check(self._lib.dygnn_tcl_forward(C.byref(cfg), C.byref(self._weights()), self.node_raw_features.data_ptr(),
                                                    self.edge_raw_features.data_ptr(), roots.data_ptr(), tms.data_ptr(), nbr.data_ptr(), eid.data_ptr(),
                                                    nts.data_ptr(), n_sides, pa.ctypes.data, pb.ctypes.data, P, out_a.data_ptr(), out_b.data_ptr(),
                                                    C.byref(tap_struct) if tap_struct is not None else None, ws.data_ptr(), ws.numel(),
                                                    _capi.current_stream_ptr()))
        return (out_a, out_b) if taps is None else (out_a, out_b, tap_out)
