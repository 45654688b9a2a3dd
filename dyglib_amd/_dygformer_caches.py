"""The two caches a DyGFormer model keeps for the library's kernels, as plain objects the model owns: the kernel-ready weight copy
(`PackedWeights`) and the projected feature tables built from it (`ProjectedTables`).  Both belong to the model, not to a stream: whichever
call finds one stale rebuilds it on its own stream with launches alone and leaves a mark (`built_mark`); every reader orders its stream
after that mark (`order_after`).  Both reach the library through `model._lib` at call time.

Which library call refreshes the weight copy is `pack_action`'s verdict:

  "keep"      the parameters are the ones packed (same addresses and version counters, same device): nothing to do
  "pack"      first call, or an address changed: dygnn_dygformer_pack (descriptor tables from the host; it synchronises its stream)
  "repack"    values changed in place, as by an optimizer step (the fragment descriptors in the buffer stay valid): dygnn_dygformer_repack,
              launches only, so no host synchronisation inside a training loop.  From the training path it is `fused_only` -- the fragment
              streams the training kernels read -- and leaves the inference sections stale (the copy is then not "complete")
  "complete"  an inference call on such a copy: the repack of the inference sections, on the unchanged key
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _capi, _glue


def built_mark(dev):
    """(stream, event recorded on it now): what a cache keeps of the stream that has just queued its build."""
    stream = torch.cuda.current_stream(dev)
    ev = torch.cuda.Event()
    ev.record(stream)
    return stream.cuda_stream, ev


def order_after(mark, dev) -> None:
    """Make the current stream wait for a cache's build when another stream queued it (hipStreamWaitEvent: nothing blocks the host)."""
    if mark is not None:
        stream = torch.cuda.current_stream(dev)
        if stream.cuda_stream != mark[0]:
            stream.wait_event(mark[1])


def pack_action(have_buffer: bool, same_key: bool, same_addresses: bool, complete: bool, training: bool) -> str:
    """What a call does to the kernel-ready copy.  have_buffer: a buffer of the right size on the right device exists; same_key: the
    parameters' (address, version) pairs and the device are the stored ones; same_addresses: the parameters and the buffer are where
    they were at the last pack or repack; complete: the inference sections are current; training: the call is a training forward."""
    if not have_buffer:
        return "pack"
    if same_key:
        return "keep" if training or complete else "complete"
    return "repack" if same_addresses else "pack"


class PackedWeights:
    """The kernel-ready weight copy of one model: the ctypes view of the parameters it was packed from, the buffer, and what decides
    the next call's action (key, addresses, complete).  `generation` counts the packs and repacks: what was derived from the copy
    (the projected tables) is stale when it has moved."""

    def __init__(self):
        self.struct = None
        self.buffer: Optional[torch.Tensor] = None
        self.key = None
        self.addresses = None
        self.complete = True
        self.generation = 0
        self.built = None

    def drop(self) -> None:
        """Forget which values were packed.  The buffer and the addresses stay: the next call repacks (launches only)."""
        self.key = None

    def get(self, model, dev, training: bool = False) -> Tuple["_capi.DygformerWeights", torch.Tensor]:
        """(ctypes view of the parameters, kernel-ready copy), brought up to date on the current stream and ordered before it."""
        lib, cfg = model._lib, model._cfg
        params = model._param_list()
        key = tuple([(p.data_ptr(), p._version) for p in params]) + (str(dev),)
        buf = self.buffer
        same_key = buf is not None and self.key == key
        if same_key:                    # the stored key vouches for the buffer (size, device) and for every address
            have, same_addresses, nbytes = True, True, buf.numel()
        else:
            _glue.require_f32_params(params)
            nbytes = lib.dygnn_dygformer_packed_bytes(C.byref(cfg))
            if nbytes == 0:
                _capi.check(-1)
            have = buf is not None and buf.numel() == nbytes and buf.device == dev
            if not have:
                buf = self.buffer = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
            addresses = tuple(k[0] for k in key[:-1]) + (buf.data_ptr(),)
            same_addresses = self.addresses == addresses
        action = pack_action(have, same_key, same_addresses, self.complete, training)
        stream = _capi.current_stream_ptr()
        if action == "complete":
            _capi.check(lib.dygnn_dygformer_repack(C.byref(cfg), C.byref(self.struct), buf.data_ptr(), nbytes, 0, stream))
            self.complete = True
        elif action != "keep":
            weights = self.struct = model._weights_struct()
            self.addresses = None       # a launch that raises leaves a state that packs in full next time
            if action == "repack":
                _capi.check(lib.dygnn_dygformer_repack(C.byref(cfg), C.byref(weights), buf.data_ptr(), nbytes, 1 if training else 0, stream))
            else:
                _capi.check(lib.dygnn_dygformer_pack(C.byref(cfg), C.byref(weights), buf.data_ptr(), nbytes, stream))
            self.complete = action == "pack" or not training
            self.addresses, self.key = addresses, key
            self.generation += 1        # the projected tables of the previous weights are stale
        if action != "keep":
            # A repack is launches only, so a call on another stream has to wait for it.  The full pack of a shape the fused kernel takes ends
            # in a synchronisation of its stream, which leaves the event complete; a shape of the generic path packs with launches alone.
            self.built = built_mark(dev)
        order_after(self.built, dev)
        return self.struct, buf


class ProjectedTables:
    """The projected node / edge feature tables of one model (DyGFormer._proj_plan says which channel gets one).  They are built on the
    first inference call after the weight copy's generation moved and live until the next one, a table assignment or `drop()`."""

    def __init__(self):
        self.key = None
        self.buffers = {}
        self.mark = None

    @property
    def built(self) -> frozenset:
        """The channels ("node", "edge") a table is currently held for."""
        return frozenset(self.buffers)

    def drop(self) -> None:
        self.key, self.buffers, self.mark = None, {}, None

    def get(self, model, dev, weights, generation: int) -> Tuple[int, Optional[torch.Tensor], Optional[torch.Tensor]]:
        """(projected bits of table_flags, projected node table, projected edge table) for an inference call."""
        plan = model._proj_plan()
        if not plan:
            return 0, None, None
        key = (generation, str(dev), tuple(sorted(plan.items())))
        if self.key != key:
            new = {}
            for ch, which in enumerate(("node", "edge")):
                if which not in plan:
                    continue
                table = getattr(model, which + "_raw_features")
                if table.dtype != torch.float32 or not table.is_contiguous():
                    raise _capi.DygnnError("feature tables must be contiguous float32")
                buf = self.buffers.get(which)
                if buf is None or buf.numel() != plan[which] or buf.device != dev:
                    buf = torch.empty(plan[which], dtype=torch.uint8, device=dev)
                _capi.check(model._lib.dygnn_dygformer_project_table(C.byref(model._cfg), C.byref(weights), ch, table.data_ptr(), int(table.shape[0]),
                                                                     buf.data_ptr(), buf.numel(), _capi.current_stream_ptr()))
                new[which] = buf
            # the build is launches only: a call on another stream must not read the tables before it ran
            self.key, self.buffers, self.mark = key, new, built_mark(dev)
        order_after(self.mark, dev)
        return model._proj_flags(plan), self.buffers.get("node"), self.buffers.get("edge")
