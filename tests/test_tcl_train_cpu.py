"""The TCL training entry points without a GPU (ctypes, in the style of test_tcl_cpu.py): the exported symbols, dygnn_tcl_train_workspace_bytes
and the host-side argument checks of dygnn_tcl_train_forward / dygnn_tcl_backward.  No kernel is launched: every call here fails validation
first, or has an empty batch."""
import ctypes as C
import os

import pytest

from dyglib_amd import _capi
from tests.test_tcl_cpu import REFUSED, SUPPORTED, config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dygnn_tcl_train_workspace_bytes", "dygnn_tcl_train_forward", "dygnn_tcl_backward")


def test_symbols_are_exported_and_declared():
    lib = _capi.load()
    header = open(os.path.join(ROOT, "include", "dygnn.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _capi.SIGNATURES and f" {name}(" in header


@pytest.mark.parametrize("kw,rc,msg", REFUSED, ids=[f"{i}" for i in range(len(REFUSED))])
def test_refused_configs(kw, rc, msg):
    lib = _capi.load()
    cfg = config(**kw)
    assert lib.dygnn_tcl_train_workspace_bytes(C.byref(cfg), 200) == 0
    assert msg in lib.dygnn_last_error().decode()
    # both entry points refuse the same way before they look at any pointer
    assert lib.dygnn_tcl_train_forward(C.byref(cfg), None, None, None, None, None, None, None, None, 5, 0.1, 1, None, None, None, 0, None) == rc
    assert msg in lib.dygnn_last_error().decode()
    assert lib.dygnn_tcl_backward(C.byref(cfg), None, None, None, None, 5, 0.1, 1, None, 0, None) == rc
    assert msg in lib.dygnn_last_error().decode()


@pytest.mark.parametrize("kw", SUPPORTED, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_workspace_bytes_of_supported_configs(kw):
    lib = _capi.load()
    cfg = config(**kw)
    last = 0
    for B in (0, 1, 2, 7, 200, 201, 1537):
        b = lib.dygnn_tcl_train_workspace_bytes(C.byref(cfg), B)
        assert b >= last and b > 0, (B, b, last)                                      # non-decreasing in batch
        last = b
        # the saved activations and the backward's scratch come on top of everything the inference forward keeps for 2 B sides, B pairs
        assert b > lib.dygnn_tcl_workspace_bytes(C.byref(cfg), 2 * B, B), B
        S, d, L = cfg.num_neighbors + 1, cfg.node_feat_dim, cfg.num_layers
        rows = 2 * max(B, 1) * S
        assert b >= 4 * rows * (d + 2 * L * (12 * d + cfg.num_heads * S))             # X0 and, per stage, 12 d floats per row plus the softmax
    assert lib.dygnn_tcl_train_workspace_bytes(C.byref(cfg), -1) == 0 and b"batch" in lib.dygnn_last_error()


def weights(layers=2):
    w = _capi.TclWeights()
    for f, _ in _capi.TclWeights._fields_:
        if f != "layers":
            setattr(w, f, 64)
    for l in range(layers):
        for f, _ in _capi.TclLayerWeights._fields_:
            setattr(w.layers[l], f, 64)
    return w


def test_train_forward_argument_checks():
    lib = _capi.load()
    cfg = config()
    fwd = lambda w, ptrs, B, p, out, ws, nbytes: lib.dygnn_tcl_train_forward(C.byref(cfg), w, *ptrs, B, p, 7, *out, ws, nbytes, None)
    nothing, dev = (None,) * 7, (64,) * 7
    assert fwd(None, nothing, 0, 0.1, (None, None), None, 0) == 0                       # empty batch: nothing to do
    assert fwd(None, nothing, -1, 0.1, (None, None), None, 0) == -1 and b"batch" in lib.dygnn_last_error()
    assert fwd(None, nothing, 2, 0.1, (None, None), None, 0) == -1 and b"null weights" in lib.dygnn_last_error()
    w = weights(layers=1)
    assert fwd(C.byref(w), nothing, 2, 0.1, (None, None), None, 0) == -1 and b"null weights (layer 1)" in lib.dygnn_last_error()
    w = weights()
    assert fwd(C.byref(w), nothing, 2, 0.1, (None, None), None, 0) == -1 and b"null pointer" in lib.dygnn_last_error()
    assert fwd(C.byref(w), dev, 2, 0.1, (64, None), 64, 1 << 40) == -1 and b"null pointer" in lib.dygnn_last_error()
    assert fwd(C.byref(w), dev, 2, 1.0, (64, 64), 64, 1 << 40) == -1 and b"dropout must be in [0, 1)" in lib.dygnn_last_error()
    assert fwd(C.byref(w), dev, 2, -0.5, (64, 64), 64, 1 << 40) == -1
    need = lib.dygnn_tcl_train_workspace_bytes(C.byref(cfg), 2)
    assert fwd(C.byref(w), dev, 2, 0.1, (64, 64), 64, need - 1) == -4 and b"workspace too small" in lib.dygnn_last_error()
    assert fwd(C.byref(w), dev, 2, 0.1, (64, 64), 64, 100) == -4


def test_backward_argument_checks():
    lib = _capi.load()
    cfg = config()
    bwd = lambda w, g, go, B, p, ws, nbytes: lib.dygnn_tcl_backward(C.byref(cfg), w, g, *go, B, p, 7, ws, nbytes, None)
    assert bwd(None, None, (None, None), 0, 0.1, None, 0) == 0
    assert bwd(None, None, (None, None), -3, 0.1, None, 0) == -1
    assert bwd(None, None, (None, None), 2, 0.1, None, 0) == -1 and b"null weights" in lib.dygnn_last_error()
    w = weights()
    assert bwd(C.byref(w), None, (None, None), 2, 0.1, None, 0) == -1 and b"null gradient buffer" in lib.dygnn_last_error()
    g = weights(layers=1)
    assert bwd(C.byref(w), C.byref(g), (64, 64), 2, 0.1, 64, 1 << 40) == -1 and b"null gradient buffer (layer 1)" in lib.dygnn_last_error()
    g = weights()
    assert bwd(C.byref(w), C.byref(g), (64, None), 2, 0.1, 64, 1 << 40) == -1 and b"null pointer" in lib.dygnn_last_error()
    assert bwd(C.byref(w), C.byref(g), (64, 64), 2, 0.1, None, 1 << 40) == -1 and b"null pointer" in lib.dygnn_last_error()
    assert bwd(C.byref(w), C.byref(g), (64, 64), 2, 1.5, 64, 1 << 40) == -1 and b"dropout must be in [0, 1)" in lib.dygnn_last_error()
    need = lib.dygnn_tcl_train_workspace_bytes(C.byref(cfg), 2)
    assert bwd(C.byref(w), C.byref(g), (64, 64), 2, 0.1, 64, need - 1) == -4 and b"workspace too small" in lib.dygnn_last_error()
