"""Drop-in for the reference `GraphMixer` backbone (models/GraphMixer.py:9-160): same constructor, same
`compute_src_dst_node_temporal_embeddings(src_node_ids, dst_node_ids, node_interact_times, num_neighbors, time_gap)` /
`compute_node_temporal_embeddings` / `set_neighbor_sampler` signatures, same parameter names and shapes (a reference checkpoint
loads with strict=True); the forward runs in libdygnn_hip.so (`dygnn_graphmixer_forward`, dyglib_amd/csrc/graphmixer.hip).

Inference (eval or train mode under torch.no_grad()) takes `dygnn_graphmixer_forward`.  Training (train mode with autograd recording) takes
`dygnn_graphmixer_train_forward` / `dygnn_graphmixer_backward` (dyglib_amd/csrc/graphmixer_train.hip) through `_GraphMixerTrainFunction`:
dropout `self.dropout` from the counter-based generator of dropout.h; every parameter receives a gradient except the frozen time encoder,
whose `.grad` stays None as in the reference; the feature tables receive none.  Eval mode with autograd recording, `compute_step_embeddings`
(the evaluation step) and `taps` with autograd recording raise NotImplementedError.  `recent` neighbour sampling only, on both paths: a
sampler with a random strategy raises NotImplementedError (the reference's evaluation forces `recent` for GraphMixer,
evaluate_models_utils.py, and its training default is `recent`).

The node encoder's `time_gap` most recent neighbours are read straight from the temporal CSR inside the kernel: no [n, time_gap] array
exists on the host or on the device, and the call's workspace (n (K C + F_n) floats) does not depend on time_gap."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _capi, _glue
from .modules import TimeEncoder
from .neighbor_sampler import NeighborSampler


class _GraphMixerTrainFunction(torch.autograd.Function):
    """compute_node_temporal_embeddings with gradients: forward = dygnn_graphmixer_train_forward, backward = dygnn_graphmixer_backward.  The
    parameters are passed as inputs only so that autograd routes their gradients; the workspace belongs to this one call (a training step
    issues a negative and a positive call before one backward())."""

    @staticmethod
    def forward(ctx, model, nodes, tms, num_neighbors, time_gap, dropout_p, seed, *params):
        dev = model.output_layer.weight.device
        n = nodes.numel()
        out = torch.empty((n, model.node_feat_dim), dtype=torch.float32, device=dev)
        ctx.model, ctx.n = model, n
        if n == 0:                                                           # nothing to launch, here or in backward
            return out
        lib = model._lib
        cfg, w = model._config(num_neighbors, time_gap), model._weights()
        nbytes = lib.dygnn_graphmixer_train_workspace_bytes(C.byref(cfg), n)
        if nbytes == 0:                                  # AssertionError (bad argument) or NotImplementedError (unsupported) with the library's message
            _capi.check(lib.dygnn_graphmixer_check(C.byref(cfg)))
            _capi.check(-1)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)          # lives until this call's backward
        _capi.check(lib.dygnn_graphmixer_train_forward(C.byref(cfg), C.byref(w), model.neighbor_sampler.csr.on_device(dev),
                                                       model.node_raw_features.data_ptr(), model.edge_raw_features.data_ptr(), nodes.data_ptr(),
                                                       tms.data_ptr(), n, float(dropout_p), int(seed), out.data_ptr(), ws.data_ptr(), nbytes,
                                                       _capi.current_stream_ptr()))
        ctx.cfg, ctx.w, ctx.ws, ctx.dropout_p, ctx.seed = cfg, w, ws, float(dropout_p), int(seed)
        ctx.param_versions = _glue.param_versions(params)
        return out

    @staticmethod
    def backward(ctx, g_out):
        model = ctx.model
        params = list(model.parameters())
        if ctx.n == 0:
            return (None,) * (7 + len(params))
        dev = ctx.ws.device
        g_out = _glue.grad_or_zeros(g_out, (ctx.n, model.node_feat_dim), dev)
        _glue.check_param_versions(params, ctx.param_versions, "GraphMixer")
        trainable = [p for p in params if p.requires_grad]                    # the time encoder is frozen: no buffer, None below
        grads = {id(p): g for p, g in zip(trainable, _glue.zero_grads(trainable, dev))}
        gstruct = model._weights(grads)
        _capi.check(model._lib.dygnn_graphmixer_backward(C.byref(ctx.cfg), C.byref(ctx.w), C.byref(gstruct), g_out.data_ptr(), ctx.n, ctx.dropout_p,
                                                         ctx.seed, ctx.ws.data_ptr(), ctx.ws.numel(), _capi.current_stream_ptr()))
        ctx.ws = None
        return (None,) * 7 + tuple(grads.get(id(p)) for p in params)


class FeedForwardNet(nn.Module):
    """Parameters of models/GraphMixer.py:163-191: ffn.0 = Linear(d, int(factor * d)), ffn.3 = Linear(int(factor * d), d)."""

    def __init__(self, input_dim: int, dim_expansion_factor: float, dropout: float = 0.0):
        super().__init__()
        self.input_dim, self.dim_expansion_factor, self.dropout = input_dim, dim_expansion_factor, dropout
        hidden = int(dim_expansion_factor * input_dim)
        self.ffn = nn.Sequential(nn.Linear(input_dim, hidden), nn.GELU(), nn.Dropout(dropout), nn.Linear(hidden, input_dim), nn.Dropout(dropout))


class MLPMixer(nn.Module):
    """Parameters of models/GraphMixer.py:194-244."""

    def __init__(self, num_tokens: int, num_channels: int, token_dim_expansion_factor: float = 0.5, channel_dim_expansion_factor: float = 4.0,
                 dropout: float = 0.0):
        super().__init__()
        self.token_norm = nn.LayerNorm(num_tokens)
        self.token_feedforward = FeedForwardNet(num_tokens, token_dim_expansion_factor, dropout)
        self.channel_norm = nn.LayerNorm(num_channels)
        self.channel_feedforward = FeedForwardNet(num_channels, channel_dim_expansion_factor, dropout)


class GraphMixer(nn.Module):

    def __init__(self, node_raw_features: np.ndarray, edge_raw_features: np.ndarray, neighbor_sampler: NeighborSampler,
                 time_feat_dim: int, num_tokens: int, num_layers: int = 2, token_dim_expansion_factor: float = 0.5,
                 channel_dim_expansion_factor: float = 4.0, dropout: float = 0.1, device: str = "cpu"):
        super().__init__()
        self.node_raw_features = torch.from_numpy(np.ascontiguousarray(node_raw_features, dtype=np.float32)).to(device)
        self.edge_raw_features = torch.from_numpy(np.ascontiguousarray(edge_raw_features, dtype=np.float32)).to(device)
        self.neighbor_sampler = neighbor_sampler
        self.node_feat_dim = self.node_raw_features.shape[1]
        self.edge_feat_dim = self.edge_raw_features.shape[1]
        self.time_feat_dim = time_feat_dim
        self.num_tokens = num_tokens
        self.num_layers = num_layers
        self.token_dim_expansion_factor = token_dim_expansion_factor
        self.channel_dim_expansion_factor = channel_dim_expansion_factor
        self.dropout = dropout
        self.device = device
        self.num_channels = self.edge_feat_dim
        self.time_encoder = TimeEncoder(time_dim=time_feat_dim, parameter_requires_grad=False)      # frozen, but part of the state_dict
        self.projection_layer = nn.Linear(self.edge_feat_dim + time_feat_dim, self.num_channels)
        self.mlp_mixers = nn.ModuleList([MLPMixer(self.num_tokens, self.num_channels, token_dim_expansion_factor, channel_dim_expansion_factor, dropout)
                                         for _ in range(num_layers)])
        self.output_layer = nn.Linear(self.num_channels + self.node_feat_dim, self.node_feat_dim, bias=True)
        self._lib = _capi.load()
        self._workspace: Dict[tuple, torch.Tensor] = {}

    def set_neighbor_sampler(self, neighbor_sampler: NeighborSampler):
        """models/GraphMixer.py:152-160."""
        _glue.reset_sampler(self, neighbor_sampler)

    # ---- the reference's entry points ------------------------------------------------------------------------------------------
    def compute_src_dst_node_temporal_embeddings(self, src_node_ids, dst_node_ids, node_interact_times, num_neighbors: int = 20,
                                                 time_gap: int = 2000) -> Tuple[torch.Tensor, torch.Tensor]:
        """models/GraphMixer.py:52-68: two float32 tensors [B, node_feat_dim]; ONE library call on the roots [src ; dst].
        In train mode with autograd recording the call is differentiable (dropout self.dropout)."""
        (src, dst), tms = self._inputs((src_node_ids, dst_node_ids), node_interact_times, trainable=True)
        B = src.numel()
        nodes, tms = torch.cat([src, dst]), torch.cat([tms, tms])
        if self.training and torch.is_grad_enabled():
            out = self._train_forward(nodes, tms, num_neighbors, time_gap)
        else:
            out = self._forward(nodes, tms, num_neighbors, time_gap)
        return out[:B], out[B:]

    def compute_node_temporal_embeddings(self, node_ids, node_interact_times, num_neighbors: int = 20, time_gap: int = 2000,
                                         taps: Optional[int] = None):
        """models/GraphMixer.py:70-150: [n, node_feat_dim].  `taps` = r (not in the reference): also return the intermediates of the first r
        roots, (embeddings, dict(projection, layer_out, token_mean, node_term)), for the parity tests.
        In train mode with autograd recording the call is differentiable (dropout self.dropout; `taps` are refused there)."""
        (nodes,), tms = self._inputs((node_ids,), node_interact_times, trainable=taps is None)
        if self.training and torch.is_grad_enabled():
            return self._train_forward(nodes, tms, num_neighbors, time_gap)
        return self._forward(nodes, tms, num_neighbors, time_gap, taps)

    def compute_step_embeddings(self, src_node_ids, dst_node_ids, neg_dst_node_ids, node_interact_times, num_neighbors: int = 20,
                                time_gap: int = 2000) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The positive and the negative call of an evaluation step (evaluate_models_utils.py:126-136) as ONE library call on the roots
        [sources ; destinations ; negative destinations] at the batch times: the negative call's sources are the positive call's (:62-63), and a
        root's row does not depend on the other roots of the call, so the three results are bit-identical to those of the two reference calls."""
        (src, dst, neg), tms = self._inputs((src_node_ids, dst_node_ids, neg_dst_node_ids), node_interact_times)
        B = src.numel()
        out = self._forward(torch.cat([src, dst, neg]), torch.cat([tms, tms, tms]), num_neighbors, time_gap)
        return out[:B], out[B:2 * B], out[2 * B:]

    # ---- glue ------------------------------------------------------------------------------------------------------------------------
    def _inputs(self, id_arrays, node_interact_times, trainable: bool = False):
        """Refuse what is not built (autograd recording outside the training calls, random sampling, a CPU model), validate host ids like the
        reference (IndexError), and move ids (int64) and times (float64) to the model's device.  `trainable`: the caller has a differentiable
        path for train mode."""
        _glue.refuse_untrainable(self, trainable, "this GraphMixer call is inference-only on the HIP path: call it under torch.no_grad().  Gradients "
                                 "flow through compute_src_dst_node_temporal_embeddings and compute_node_temporal_embeddings (without taps) in "
                                 "train mode only (eval mode and compute_step_embeddings have no backward pass)")
        self.neighbor_sampler._check_strategy()
        if self.neighbor_sampler.sample_neighbor_strategy != "recent":
            raise NotImplementedError(f"GraphMixer on the HIP path samples on the device and supports sample_neighbor_strategy 'recent' only, not "
                                      f"'{self.neighbor_sampler.sample_neighbor_strategy}'")
        dev = self.output_layer.weight.device
        _glue.require_cuda_tables(self, dev)
        n_nodes = self.node_raw_features.shape[0]
        _glue.validate_ids(self, self.neighbor_sampler.csr, id_arrays, n_nodes, n_nodes, self.edge_raw_features.shape[0])
        parts = [_glue.to_dev(ids, torch.int64, dev).reshape(-1) for ids in id_arrays]
        tms = _glue.to_dev(node_interact_times, torch.float64, dev).reshape(-1)
        assert all(p.numel() == tms.numel() for p in parts)
        return parts, tms

    def _config(self, num_neighbors: int, time_gap: int) -> "_capi.GraphmixerConfig":
        K, Cc = self.num_tokens, self.num_channels
        return _capi.GraphmixerConfig(self.node_feat_dim, self.edge_feat_dim, self.time_feat_dim, K, self.num_layers,
                                      int(self.token_dim_expansion_factor * K), int(self.channel_dim_expansion_factor * Cc),      # as FeedForwardNet
                                      int(num_neighbors), int(time_gap), self.node_raw_features.shape[0])

    def _weights(self, replace: Optional[dict] = None) -> "_capi.GraphmixerWeights":
        """ctypes view of the parameters; `replace` maps id(parameter) to another tensor of the same shape (the gradient buffers of the
        backward pass; a parameter it does not name, the frozen time encoder, becomes NULL)."""
        _glue.require_f32_params(self.parameters())
        w = _capi.GraphmixerWeights()
        p = (lambda t: t.data_ptr()) if replace is None else (lambda t: replace[id(t)].data_ptr() if id(t) in replace else None)
        w.time_w, w.time_b = p(self.time_encoder.w.weight), p(self.time_encoder.w.bias)
        w.proj_w, w.proj_b = p(self.projection_layer.weight), p(self.projection_layer.bias)
        for l, m in enumerate(self.mlp_mixers):
            L, tf, cf = w.layers[l], m.token_feedforward.ffn, m.channel_feedforward.ffn
            L.token_norm_w, L.token_norm_b = p(m.token_norm.weight), p(m.token_norm.bias)
            L.token_fc0_w, L.token_fc0_b, L.token_fc1_w, L.token_fc1_b = p(tf[0].weight), p(tf[0].bias), p(tf[3].weight), p(tf[3].bias)
            L.channel_norm_w, L.channel_norm_b = p(m.channel_norm.weight), p(m.channel_norm.bias)
            L.channel_fc0_w, L.channel_fc0_b, L.channel_fc1_w, L.channel_fc1_b = p(cf[0].weight), p(cf[0].bias), p(cf[3].weight), p(cf[3].bias)
        w.output_w, w.output_b = p(self.output_layer.weight), p(self.output_layer.bias)
        return w

    def _train_forward(self, nodes: torch.Tensor, tms: torch.Tensor, num_neighbors: int, time_gap: int) -> torch.Tensor:
        if self.num_layers > _capi.DYGNN_MAX_LAYERS or len(self.mlp_mixers) != self.num_layers:
            raise NotImplementedError(f"graphmixer: num_layers {self.num_layers} not supported (1..{_capi.DYGNN_MAX_LAYERS})")
        return _GraphMixerTrainFunction.apply(self, nodes, tms, int(num_neighbors), int(time_gap), float(self.dropout), _glue.dropout_seed(self),
                                              *self.parameters())

    def _forward(self, nodes: torch.Tensor, tms: torch.Tensor, num_neighbors: int, time_gap: int, taps: Optional[int] = None):
        dev = nodes.device
        n = nodes.numel()
        cfg = self._config(num_neighbors, time_gap)
        if self.num_layers > _capi.DYGNN_MAX_LAYERS or len(self.mlp_mixers) != self.num_layers:
            raise NotImplementedError(f"graphmixer: num_layers {self.num_layers} not supported (1..{_capi.DYGNN_MAX_LAYERS})")
        nbytes = self._lib.dygnn_graphmixer_workspace_bytes(C.byref(cfg), n)
        if nbytes == 0:                                  # AssertionError (bad argument) or NotImplementedError (unsupported) with the library's message
            _capi.check(self._lib.dygnn_graphmixer_check(C.byref(cfg)))
        ws = _glue.workspace(self._workspace, nbytes, n, num_neighbors, dev)
        out = torch.empty((n, self.node_feat_dim), dtype=torch.float32, device=dev)
        tap_struct, tap_out = None, None
        if taps is not None:
            r, K, Cc = min(int(taps), n), self.num_tokens, self.num_channels
            new = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
            tap_out = dict(projection=new(r, K, Cc), layer_out=[new(r, K, Cc) for _ in range(self.num_layers)], token_mean=new(r, Cc),
                           node_term=new(r, self.node_feat_dim))
            tap_struct = _capi.GraphmixerTaps()
            tap_struct.rows = r
            tap_struct.projection, tap_struct.token_mean, tap_struct.node_term = (tap_out[k].data_ptr() for k in ("projection", "token_mean", "node_term"))
            for l, t in enumerate(tap_out["layer_out"]):
                tap_struct.layer_out[l] = t.data_ptr()
        if n > 0:
            _capi.check(self._lib.dygnn_graphmixer_forward(C.byref(cfg), C.byref(self._weights()), self.neighbor_sampler.csr.on_device(dev),
                                                           self.node_raw_features.data_ptr(), self.edge_raw_features.data_ptr(), nodes.data_ptr(),
                                                           tms.data_ptr(), n, out.data_ptr(), C.byref(tap_struct) if tap_struct is not None else None,
                                                           ws.data_ptr(), ws.numel(), _capi.current_stream_ptr()))
        return out if taps is None else (out, tap_out)
