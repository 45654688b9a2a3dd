"""Drop-in for the reference `CAWN` backbone (models/CAWN.py:10-396): same constructor, same
`compute_src_dst_node_temporal_embeddings(src_node_ids, dst_node_ids, node_interact_times, num_neighbors)` / `set_neighbor_sampler`
signatures, same parameter names and shapes (a reference checkpoint loads with strict=True); the forward runs in libdygnn_hip.so
(`dygnn_cawn_forward`, dyglib_amd/csrc/cawn.hip).

Inference (eval mode, or train mode under torch.no_grad()) takes `dygnn_cawn_forward`.  Training is OPT-IN: after `enable_training()`, a call
in train mode with autograd recording takes `dygnn_cawn_train_forward` / `dygnn_cawn_backward` (dyglib_amd/csrc/cawn_train.hip) through
`_CawnTrainFunction`: dropout `self.dropout` from the counter-based generator of dropout.h, every parameter receives a gradient (the reverse
directions' weight_hh an exactly zero one), the feature tables do not.  Without `enable_training()` a call with autograd recording raises
NotImplementedError, as do, with or without it, eval mode, `compute_step_embeddings` and `taps=` with autograd recording.  All three
neighbour sampling strategies work on both paths: the hops are sampled by `NeighborSampler.get_historical_neighbors_device` in the
reference's call order (all hops of the sources, then all hops of the destinations, hop h >= 2 queried at the float32 times of hop h - 1)
and handed to the library.

In CAWN the source embedding depends on the destination it is paired with (the position features count appearances in both trees), so an
evaluation step has FOUR results: `compute_step_embeddings` returns (src of the positive call, dst, src of the negative call, neg_dst)."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _capi, _glue
from .modules import TimeEncoder, TransformerEncoder, fill_encoder_layer_weights
from .neighbor_sampler import NeighborSampler


class _CawnTrainFunction(torch.autograd.Function):
    """compute_src_dst_node_temporal_embeddings with gradients: forward = dygnn_cawn_train_forward, backward = dygnn_cawn_backward.  The
    parameters are passed as inputs only so that autograd routes their gradients; the workspace belongs to this one call (a training step
    issues a negative and a positive call before one backward())."""

    @staticmethod
    def forward(ctx, model, sides, B, num_neighbors, dropout_p, seed, *params):
        dev = model.walk_encoder.projection_layers[1].weight.device
        d = model.node_feat_dim
        out = (torch.empty((B, d), dtype=torch.float32, device=dev), torch.empty((B, d), dtype=torch.float32, device=dev))
        ctx.model, ctx.B = model, B
        if B == 0:                                                           # nothing to launch, here or in backward
            return out
        lib = model._lib
        cfg, w = model._config(num_neighbors), model._weights()
        nbytes = lib.dygnn_cawn_train_workspace_bytes(C.byref(cfg), B)
        if nbytes == 0:                                  # AssertionError (bad argument) or NotImplementedError (unsupported) with the library's message
            msg = lib.dygnn_last_error().decode("utf-8", "replace")
            _capi.check(lib.dygnn_cawn_check(C.byref(cfg)))
            raise NotImplementedError(msg) if "not supported" in msg else AssertionError(msg)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)          # lives until this call's backward
        roots, tms, hops = sides
        h = _capi.CawnHops()
        for i, (n, e, t) in enumerate(hops):
            h.id[i], h.eid[i], h.t[i] = n.data_ptr(), e.data_ptr(), t.data_ptr()
        _capi.check(lib.dygnn_cawn_train_forward(C.byref(cfg), C.byref(w), model.node_raw_features.data_ptr(), model.edge_raw_features.data_ptr(),
                                                 roots.data_ptr(), tms.data_ptr(), C.byref(h), B, float(dropout_p), int(seed), out[0].data_ptr(),
                                                 out[1].data_ptr(), ws.data_ptr(), nbytes, _capi.current_stream_ptr()))
        ctx.cfg, ctx.w, ctx.ws, ctx.dropout_p, ctx.seed = cfg, w, ws, float(dropout_p), int(seed)
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
        _glue.check_param_versions(params, ctx.param_versions, "CAWN")
        grads = _glue.zero_grads(params, dev, align_floats=4)                  # the library's products read the buffers as float4
        gstruct = model._weights({id(p): g for p, g in zip(params, grads)})
        _capi.check(model._lib.dygnn_cawn_backward(C.byref(ctx.cfg), C.byref(ctx.w), C.byref(gstruct), g_src.data_ptr(), g_dst.data_ptr(), ctx.B,
                                                   ctx.dropout_p, ctx.seed, ctx.ws.data_ptr(), ctx.ws.numel(), _capi.current_stream_ptr()))
        ctx.ws = None
        return (None,) * 6 + tuple(grads)


class PositionEncoder(nn.Module):
    """Parameters of models/CAWN.py:178-195."""

    def __init__(self, position_feat_dim: int, walk_length: int, device: str = "cpu"):
        super().__init__()
        self.position_feat_dim = position_feat_dim
        self.walk_length = walk_length
        self.device = device
        self.position_encode_layer = nn.Sequential(nn.Linear(self.walk_length + 1, self.position_feat_dim), nn.ReLU(),
                                                   nn.Linear(self.position_feat_dim, self.position_feat_dim))


class BiLSTMEncoder(nn.Module):
    """Parameters of models/CAWN.py:358-369."""

    def __init__(self, input_dim: int, hidden_dim: int):
        super().__init__()
        self.hidden_dim_one_direction = hidden_dim // 2
        self.model_dim = self.hidden_dim_one_direction * 2
        self.bilstm_encoder = nn.LSTM(input_size=input_dim, hidden_size=self.hidden_dim_one_direction, batch_first=True, bidirectional=True)


class WalkEncoder(nn.Module):
    """Parameters of models/CAWN.py:292-328."""

    def __init__(self, input_dim: int, position_feat_dim: int, output_dim: int, num_walk_heads: int, dropout: float = 0.1):
        super().__init__()
        self.input_dim = input_dim
        self.position_feat_dim = position_feat_dim
        self.attention_dim = self.input_dim // 2
        self.output_dim = output_dim
        self.num_walk_heads = num_walk_heads
        self.dropout = dropout
        if self.attention_dim % self.num_walk_heads != 0:
            self.attention_dim += (self.num_walk_heads - self.attention_dim % self.num_walk_heads)
        self.feature_encoder = BiLSTMEncoder(input_dim=self.input_dim, hidden_dim=self.input_dim)
        self.position_encoder = BiLSTMEncoder(input_dim=self.position_feat_dim, hidden_dim=self.position_feat_dim)
        self.transformer_encoder = TransformerEncoder(attention_dim=self.attention_dim, num_heads=self.num_walk_heads, dropout=self.dropout)
        self.projection_layers = nn.ModuleList([
            nn.Linear(self.feature_encoder.model_dim + self.position_encoder.model_dim, self.attention_dim),
            nn.Linear(self.attention_dim, self.output_dim)])


class CAWN(nn.Module):

    def __init__(self, node_raw_features: np.ndarray, edge_raw_features: np.ndarray, neighbor_sampler: NeighborSampler,
                 time_feat_dim: int, position_feat_dim: int, walk_length: int = 2, num_walk_heads: int = 8, dropout: float = 0.1, device: str = "cpu"):
        super().__init__()
        self.node_raw_features = torch.from_numpy(np.ascontiguousarray(node_raw_features, dtype=np.float32)).to(device)
        self.edge_raw_features = torch.from_numpy(np.ascontiguousarray(edge_raw_features, dtype=np.float32)).to(device)
        self.neighbor_sampler = neighbor_sampler
        self.node_feat_dim = self.node_raw_features.shape[1]
        self.edge_feat_dim = self.edge_raw_features.shape[1]
        self.time_feat_dim = time_feat_dim
        self.position_feat_dim = position_feat_dim
        self.walk_length = walk_length
        self.num_walk_heads = num_walk_heads
        self.dropout = dropout
        self.device = device
        self.time_encoder = TimeEncoder(time_dim=time_feat_dim)
        self.position_encoder = PositionEncoder(position_feat_dim=self.position_feat_dim, walk_length=self.walk_length, device=device)
        self.walk_encoder = WalkEncoder(input_dim=self.node_feat_dim + self.edge_feat_dim + self.time_feat_dim + self.position_feat_dim,
                                        position_feat_dim=self.position_feat_dim, output_dim=self.node_feat_dim, num_walk_heads=self.num_walk_heads,
                                        dropout=dropout)
        self._lib = _capi.load()
        self._workspace: Dict[tuple, torch.Tensor] = {}
        self._training_enabled = False

    def enable_training(self, enabled: bool = True) -> "CAWN":
        """Opt in to (or out of) the differentiable path: with it on, compute_src_dst_node_temporal_embeddings in train mode with autograd
        recording runs dygnn_cawn_train_forward and records dygnn_cawn_backward.  Off by default; returns self."""
        self._training_enabled = bool(enabled)
        return self

    def set_neighbor_sampler(self, neighbor_sampler: NeighborSampler):
        """models/CAWN.py:166-175."""
        _glue.reset_sampler(self, neighbor_sampler)

    # ---- the reference's entry point ---------------------------------------------------------------------------------------------------
    def compute_src_dst_node_temporal_embeddings(self, src_node_ids, dst_node_ids, node_interact_times, num_neighbors: int = 20,
                                                 taps: Optional[int] = None):
        """models/CAWN.py:48-80: two float32 tensors [B, node_feat_dim]; ONE library call on the sides [src ; dst] and the pairs (i, B + i).
        `taps` = r (not in the reference): also return the intermediates of the first r pairs, (src, dst, dict(walk_ids [r, 2, M, W + 1],
        counts [r, 2, M, W + 1, 2, W + 1], feature_out [r, 2, M, D], position_out [r, 2, M, P], attn_in / attn_out [r, 2, M, attention_dim]));
        index 0 / 1 of the second axis is the source / destination side.
        After enable_training(), in train mode with autograd recording, the call is differentiable (dropout self.dropout; `taps` are refused)."""
        train = self._training_enabled and self.training and torch.is_grad_enabled()
        if train and taps is not None:
            raise NotImplementedError("cawn: taps are an inference facility; the training path does not return intermediates")
        (src, dst), tms = self._inputs((src_node_ids, dst_node_ids), node_interact_times, num_neighbors, trainable=True)
        B = src.numel()
        sides = self._sample([src, dst], tms, num_neighbors)
        if train:
            return _CawnTrainFunction.apply(self, sides, B, int(num_neighbors), float(self.dropout), _glue.dropout_seed(self), *self.parameters())
        idx = np.arange(B, dtype=np.int32)
        return self._forward(sides, idx, idx + B, num_neighbors, taps)

    def compute_step_embeddings(self, src_node_ids, dst_node_ids, neg_dst_node_ids, node_interact_times, num_neighbors: int = 20
                                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """The positive and the negative call of an evaluation step (evaluate_models_utils.py:126-136) as ONE library call: (src_pos, dst,
        src_neg, neg_dst), equal to compute_src_dst...(src, dst) followed by compute_src_dst...(src, neg_dst).  With `recent` sampling the
        source walks are sampled once (sides [src ; dst ; neg_dst], 2 B pairs); a random strategy samples in the order of the reference's two
        calls (src, dst, src, neg_dst), so the sources are drawn twice and are four B sides."""
        (src, dst, neg), tms = self._inputs((src_node_ids, dst_node_ids, neg_dst_node_ids), node_interact_times, num_neighbors)
        B = src.numel()
        idx = np.arange(B, dtype=np.int32)
        if self.neighbor_sampler.sample_neighbor_strategy == "recent":
            sides = self._sample([src, dst, neg], tms, num_neighbors)
            a, b = np.concatenate([idx, idx]), np.concatenate([idx + B, idx + 2 * B])
        else:
            sides = self._sample([src, dst, src, neg], tms, num_neighbors)
            a, b = np.concatenate([idx, idx + 2 * B]), np.concatenate([idx + B, idx + 3 * B])
        oa, ob = self._forward(sides, a, b, num_neighbors)
        return oa[:B], ob[:B], oa[B:], ob[B:]

    # ---- glue ------------------------------------------------------------------------------------------------------------------------
    def _inputs(self, id_arrays, node_interact_times, num_neighbors, trainable: bool = False):
        """Refuse what is not built or not enabled (autograd recording outside the opted-in training call, a CPU model), validate host ids
        like the reference (IndexError; a target id of 0 is an AssertionError: the reference fails on it in pack_padded_sequence, its walks
        having length 0), and move ids (int64) and times (float64) to the model's device.  `trainable`: the caller has a differentiable path
        for train mode."""
        _glue.refuse_untrainable(self, trainable and self._training_enabled,
                                 "this dyglib_amd.CAWN call is inference-only on the HIP path: call it under torch.no_grad().  Gradients flow "
                                 "through compute_src_dst_node_temporal_embeddings in train mode after enable_training() only (eval mode, "
                                 "compute_step_embeddings and taps have no backward pass)")
        self.neighbor_sampler._check_strategy()
        assert num_neighbors > 0, "Number of sampled neighbors for each node should be greater than 0!"          # utils/utils.py:157
        assert self.walk_length > 0, "Number of sampled hops should be greater than 0!"                          # utils/utils.py:228
        _capi.check(self._lib.dygnn_cawn_check(C.byref(self._config(num_neighbors))))      # NotImplementedError with the library's message
        dev = self.walk_encoder.projection_layers[1].weight.device
        n_nodes = self.node_raw_features.shape[0]
        _glue.validate_ids(self, self.neighbor_sampler.csr, id_arrays, n_nodes, n_nodes, self.edge_raw_features.shape[0])
        for ids in id_arrays:
            if not isinstance(ids, torch.Tensor) and np.asarray(ids).size:
                assert int(np.asarray(ids).min()) > 0, "cawn: node id 0 is the padding node: as a target its walks have length 0"
        _glue.require_cuda_tables(self, dev)
        parts = [_glue.to_dev(ids, torch.int64, dev).reshape(-1) for ids in id_arrays]
        tms = _glue.to_dev(node_interact_times, torch.float64, dev).reshape(-1)
        assert all(p.numel() == tms.numel() for p in parts)
        return parts, tms

    def _sample(self, parts, tms, num_neighbors):
        """get_multi_hop_neighbors (utils/utils.py:216-252) per part on the device, in order (the order matters for the random strategies):
        all hops of a part before the next part -> (targets, times, per hop (ids, edge ids, times) [n_sides, k ** hop]), or None."""
        smp = self.neighbor_sampler
        if smp.device != tms.device:
            raise _capi.DygnnError(f"the neighbor sampler is on {smp.device}, the model on {tms.device}")
        if tms.numel() == 0:
            return None
        B = tms.numel()
        drawn = []
        for p in parts:
            hops = [smp.get_historical_neighbors_device(p, tms, num_neighbors)]
            for _ in range(1, self.walk_length):
                n, e, t = smp.get_historical_neighbors_device(hops[-1][0].reshape(-1), hops[-1][2].reshape(-1).double(), num_neighbors)
                hops.append((n.reshape(B, -1), e.reshape(B, -1), t.reshape(B, -1)))
            drawn.append(hops)
        cat = lambda xs: (xs[0] if len(xs) == 1 else torch.cat(xs)).contiguous()
        hops = [tuple(cat([d[h][x] for d in drawn]) for x in range(3)) for h in range(self.walk_length)]
        return cat(parts), cat([tms] * len(parts)), hops

    def _config(self, num_neighbors: int) -> "_capi.CawnConfig":
        return _capi.CawnConfig(self.node_feat_dim, self.edge_feat_dim, self.time_feat_dim, self.position_feat_dim, self.walk_length, int(num_neighbors),
                                self.num_walk_heads, self.node_raw_features.shape[0], self.edge_raw_features.shape[0])

    def _weights(self, replace: Optional[dict] = None) -> "_capi.CawnWeights":
        """ctypes view of the parameters; `replace` maps id(parameter) to another tensor of the same shape (the gradient buffers of the
        backward pass)."""
        _glue.require_f32_params(self.parameters())
        w = _capi.CawnWeights()
        p = (lambda t: t.data_ptr()) if replace is None else (lambda t: replace[id(t)].data_ptr())
        w.time_w, w.time_b = p(self.time_encoder.w.weight), p(self.time_encoder.w.bias)
        mlp = self.position_encoder.position_encode_layer
        w.pos_w0, w.pos_b0, w.pos_w1, w.pos_b1 = p(mlp[0].weight), p(mlp[0].bias), p(mlp[2].weight), p(mlp[2].bias)
        we = self.walk_encoder
        for dst, enc in ((w.feature, we.feature_encoder), (w.position, we.position_encoder)):
            for d, suffix in enumerate(("", "_reverse")):
                g = lambda name: p(getattr(enc.bilstm_encoder, name + suffix))
                dst[d].w_ih, dst[d].w_hh, dst[d].b_ih, dst[d].b_hh = g("weight_ih_l0"), g("weight_hh_l0"), g("bias_ih_l0"), g("bias_hh_l0")
        fill_encoder_layer_weights(w.attn, we.transformer_encoder, p)
        pl = we.projection_layers
        w.proj0_w, w.proj0_b, w.proj1_w, w.proj1_b = p(pl[0].weight), p(pl[0].bias), p(pl[1].weight), p(pl[1].bias)
        return w

    def _forward(self, sides, pair_a: np.ndarray, pair_b: np.ndarray, num_neighbors: int, taps: Optional[int] = None):
        dev = self.walk_encoder.projection_layers[1].weight.device
        P = len(pair_a)
        n_sides = 0 if sides is None else sides[0].numel()
        cfg = self._config(num_neighbors)
        nbytes = self._lib.dygnn_cawn_workspace_bytes(C.byref(cfg), n_sides, P)
        if nbytes == 0:                                  # AssertionError (bad argument) or NotImplementedError (unsupported) with the library's message
            _capi.check(self._lib.dygnn_cawn_check(C.byref(cfg)))
        ws = _glue.workspace(self._workspace, nbytes, (n_sides, P), num_neighbors, dev)
        d, W1, M = self.node_feat_dim, self.walk_length + 1, int(num_neighbors) ** self.walk_length
        out_a = torch.empty((P, d), dtype=torch.float32, device=dev)
        out_b = torch.empty((P, d), dtype=torch.float32, device=dev)
        tap_struct, tap_out = None, None
        if taps is not None:
            r = min(int(taps), P)
            we = self.walk_encoder
            new = lambda *shape, dtype=torch.float32: torch.zeros((r, 2, M) + shape, dtype=dtype, device=dev)
            tap_out = dict(walk_ids=new(W1, dtype=torch.int64), counts=new(W1, 2, W1), feature_out=new(we.feature_encoder.model_dim),
                           position_out=new(we.position_encoder.model_dim), attn_in=new(we.attention_dim), attn_out=new(we.attention_dim))
            tap_struct = _capi.CawnTaps()
            tap_struct.rows = r
            for k, t in tap_out.items():
                setattr(tap_struct, k, t.data_ptr())
        if P > 0:
            roots, tms, hops = sides
            h = _capi.CawnHops()
            for i, (n, e, t) in enumerate(hops):
                h.id[i], h.eid[i], h.t[i] = n.data_ptr(), e.data_ptr(), t.data_ptr()
            pa, pb = np.ascontiguousarray(pair_a, dtype=np.int32), np.ascontiguousarray(pair_b, dtype=np.int32)
            _capi.check(self._lib.dygnn_cawn_forward(C.byref(cfg), C.byref(self._weights()), self.node_raw_features.data_ptr(),
                                                     self.edge_raw_features.data_ptr(), roots.data_ptr(), tms.data_ptr(), C.byref(h), n_sides,
                                                     pa.ctypes.data, pb.ctypes.data, P, out_a.data_ptr(), out_b.data_ptr(),
                                                     C.byref(tap_struct) if tap_struct is not None else None, ws.data_ptr(), ws.numel(),
                                                     _capi.current_stream_ptr()))
        return (out_a, out_b) if taps is None else (out_a, out_b, tap_out)
