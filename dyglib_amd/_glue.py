"""Host glue that every backbone's Python mirror needs and none of them owns: plain functions, called where each class used to carry its
own copy (input upload, workspace cache, device / id / parameter checks, the dropout seed, and the three pieces of a training backward)."""
from __future__ import annotations

from typing import Dict, List

import numpy as np
import torch

from . import _capi


def to_dev(x, dtype, dev, non_blocking: bool = False) -> torch.Tensor:
    """A contiguous `dtype` tensor on `dev` from a tensor or an array-like (int64 ids, float64 times)."""
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(x, dtype={torch.int64: np.int64, torch.float64: np.float64}[dtype])).to(dev, non_blocking=non_blocking)


def workspace(cache: Dict[tuple, torch.Tensor], nbytes: int, batch: int, num_neighbors: int, dev) -> torch.Tensor:
    """The model's workspace for (batch, num_neighbors, current stream) of at least `nbytes` (0: the library refused the config)."""
    if nbytes == 0:
        _capi.check(-1)                      # AssertionError with the library's message (e.g. num_neighbors <= 0)
    key = (batch, int(num_neighbors), torch.cuda.current_stream(dev).cuda_stream)
    ws = cache.get(key)
    if ws is None or ws.numel() < nbytes or ws.device != dev:
        if len(cache) > 8:
            cache.clear()
        ws = cache[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return ws


def require_cuda_tables(model, dev) -> None:
    """Refuse a model that is not on a GPU; move its two feature tables to `dev` when they are elsewhere."""
    if dev.type != "cuda":
        raise _capi.DygnnError(f"dyglib_amd.{type(model).__name__} runs on an MI355X only; there is no CPU fallback")
    if model.node_raw_features.device != dev:
        model.node_raw_features, model.edge_raw_features = model.node_raw_features.to(dev), model.edge_raw_features.to(dev)


def validate_ids(model, csr, id_arrays, node_limit: int, node_rows: int, edge_rows: int) -> None:
    """The graph against tables of `node_rows` / `edge_rows` rows, once per sampler (every id reachable through it is inside them), and every
    query id array against `node_limit` (IndexError like the reference's indexing)."""
    if getattr(model, "_validated_csr", None) is not csr:
        csr.check_tables(node_rows, edge_rows)
        model._validated_csr = csr
    for ids in id_arrays:
        csr.check_query_ids(ids, limit=node_limit)


def reset_sampler(model, sampler) -> None:
    """The body of the reference's set_neighbor_sampler: a random strategy starts again from its seed."""
    model.neighbor_sampler = sampler
    if sampler.sample_neighbor_strategy in ["uniform", "time_interval_aware"]:
        assert sampler.seed is not None
        sampler.reset_random_state()


def refuse_untrainable(model, trainable: bool, message: str) -> None:
    """NotImplementedError(message) when autograd is recording but this call has no backward (`trainable`: it has one in train mode): the
    result would carry no graph and loss.backward() would silently do nothing."""
    if torch.is_grad_enabled() and (model.training or any(p.requires_grad for p in model.parameters())) and not (trainable and model.training):
        raise NotImplementedError(message)


def require_f32_params(params) -> None:
    for p in params:
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise _capi.DygnnError("parameters must be contiguous float32")


def dropout_seed(model) -> int:
    """The seed of a training call's dropout masks: tests pin it (`model._fixed_dropout_seed`); normally ONE draw from torch's generator, so
    torch.manual_seed governs the masks."""
    seed = getattr(model, "_fixed_dropout_seed", None)
    return int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else seed


def param_versions(params) -> list:
    """What a training forward remembers of the parameters it read (address and version counter; a write through `.data` bumps neither)."""
    return [(p.data_ptr(), p._version) for p in params]


def check_param_versions(params, saved: list, name: str) -> None:
    """The backward pass re-reads the CURRENT parameter values: they must be the ones the forward used (PyTorch raises the same way when a
    tensor saved for backward was modified in place, e.g. by an optimizer step between forward and backward)."""
    if param_versions(params) != saved:
        raise RuntimeError("one of the variables needed for gradient computation has been modified by an inplace operation: "
                           f"a {name} parameter changed between this call's forward and its backward")


def zero_grads(params, dev, align_floats: int = 1) -> List[torch.Tensor]:
    """One zero-filled float32 buffer (one fill for all gradients) as a list of view_as(p) slices in order; every slice starts at a multiple
    of `align_floats` floats (4 where the library's products read the buffers as float4)."""
    sizes = [p.numel() for p in params]
    padded = sizes if align_floats == 1 else [-(-n // align_floats) * align_floats for n in sizes]
    chunks = torch.zeros(sum(padded), dtype=torch.float32, device=dev).split(padded)
    if padded is not sizes:
        chunks = [c[:n] for c, n in zip(chunks, sizes)]
    return [c.view_as(p) for c, p in zip(chunks, params)]


def grad_or_zeros(g, shape, dev) -> torch.Tensor:
    """An incoming gradient as the library reads it: contiguous float32, zeros where autograd passed None."""
    return (g if g is not None else torch.zeros(shape, device=dev)).contiguous().float()
