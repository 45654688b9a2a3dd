"""The CAWN training entry points without a GPU (ctypes, in the style of test_tcl_train_cpu.py): the exported symbols, the ABI version,
dygnn_cawn_train_workspace_bytes, the host-side argument checks of dygnn_cawn_train_forward / dygnn_cawn_backward (no kernel is launched:
every call here fails validation first, or has an empty batch), and the opt-in switch of the drop-in class on a CPU model."""
import ctypes as C
import os

import pytest

from dyglib_amd import _capi
from tests.test_cawn_cpu import REFUSED, SUPPORTED, config, make_cpu_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dygnn_cawn_train_workspace_bytes", "dygnn_cawn_train_forward", "dygnn_cawn_backward")
MAX_TRAIN_WALKS = 64                                                 # one key per lane in the attention backward


def walks(kw):
    return kw.get("k", 32) ** kw.get("W", 1)


def test_symbols_are_exported_and_declared_and_the_abi_version_stays():
    lib = _capi.load()
    header = open(os.path.join(ROOT, "include", "dygnn.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _capi.SIGNATURES and f" {name}(" in header
    assert _capi.ABI_VERSION == 21 and lib.dygnn_abi_version() == 21      # the change only adds symbols


@pytest.mark.parametrize("kw,rc,msg", REFUSED, ids=[f"{i}" for i in range(len(REFUSED))])
def test_refused_configs(kw, rc, msg):
    """whatever dygnn_cawn_check refuses, the training path refuses with the same message, before it looks at any pointer"""
    lib = _capi.load()
    cfg = config(**kw)
    assert lib.dygnn_cawn_train_workspace_bytes(C.byref(cfg), 200) == 0
    assert msg in lib.dygnn_last_error().decode()
    assert lib.dygnn_cawn_train_forward(C.byref(cfg), None, None, None, None, None, None, 5, 0.1, 1, None, None, None, 0, None) == rc
    assert msg in lib.dygnn_last_error().decode()
    assert lib.dygnn_cawn_backward(C.byref(cfg), None, None, None, None, 5, 0.1, 1, None, 0, None) == rc
    assert msg in lib.dygnn_last_error().decode()


@pytest.mark.parametrize("kw", SUPPORTED, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()) or "wikipedia")
def test_workspace_bytes_of_supported_configs(kw):
    lib = _capi.load()
    cfg = config(**kw)
    if walks(kw) > MAX_TRAIN_WALKS:                                   # accepted by the inference forward, refused here, naming the value
        assert lib.dygnn_cawn_train_workspace_bytes(C.byref(cfg), 200) == 0
        assert f"{walks(kw)} walks" in lib.dygnn_last_error().decode() and "> 64 not supported by the training path" in lib.dygnn_last_error().decode()
        assert lib.dygnn_cawn_train_forward(C.byref(cfg), None, None, None, None, None, None, 5, 0.1, 1, None, None, None, 0, None) == -3
        assert lib.dygnn_cawn_backward(C.byref(cfg), None, None, None, None, 5, 0.1, 1, None, 0, None) == -3
        return
    last = 0
    for B in (0, 1, 2, 7, 200, 201, 1537):
        b = lib.dygnn_cawn_train_workspace_bytes(C.byref(cfg), B)
        assert b >= last and b > 0, (B, b, last)                                      # non-decreasing in batch
        last = b
        # the saved activations and the backward's scratch come on top of everything the inference forward keeps for 2 B sides, B pairs
        assert b > lib.dygnn_cawn_workspace_bytes(C.byref(cfg), 2 * B, B), B
    assert lib.dygnn_cawn_train_workspace_bytes(C.byref(cfg), -1) == 0 and b"batch" in lib.dygnn_last_error()


def weights():
    w = _capi.CawnWeights()
    for f, t in _capi.CawnWeights._fields_:
        if t is C.c_void_p:
            setattr(w, f, 64)
    for enc in (w.feature, w.position):
        for d in range(2):
            for f, _ in _capi.CawnLstmWeights._fields_:
                setattr(enc[d], f, 64)
    for f, _ in _capi.TclLayerWeights._fields_:
        setattr(w.attn, f, 64)
    return w


def test_train_forward_argument_checks():
    lib = _capi.load()
    cfg = config(W=2, k=4, P=24, heads=4)
    fwd = lambda w, ptrs, B, p, out, ws, nbytes: lib.dygnn_cawn_train_forward(C.byref(cfg), w, *ptrs, B, p, 7, *out, ws, nbytes, None)
    nothing = (None,) * 5
    assert fwd(None, nothing, 0, 0.1, (None, None), None, 0) == 0                       # empty batch: nothing to do
    assert fwd(None, nothing, -1, 0.1, (None, None), None, 0) == -1 and b"batch" in lib.dygnn_last_error()
    assert fwd(None, nothing, 2, 0.1, (None, None), None, 0) == -1 and b"null weights" in lib.dygnn_last_error()
    w = weights()
    w.position[1].b_hh = None
    assert fwd(C.byref(w), nothing, 2, 0.1, (None, None), None, 0) == -1 and b"null weights (an LSTM tensor, direction 1)" in lib.dygnn_last_error()
    w = weights()
    w.attn.norm1_b = None
    assert fwd(C.byref(w), nothing, 2, 0.1, (None, None), None, 0) == -1 and b"null weights (a transformer tensor)" in lib.dygnn_last_error()
    w = weights()
    assert fwd(C.byref(w), nothing, 2, 0.1, (None, None), None, 0) == -1 and b"null pointer" in lib.dygnn_last_error()
    hops = _capi.CawnHops()
    hops.id[0] = hops.eid[0] = hops.t[0] = 64
    dev = (64, 64, 64, 64, C.byref(hops))
    assert fwd(C.byref(w), dev, 2, 0.1, (64, 64), 64, 1 << 40) == -1 and b"null pointer (hop 2 arrays)" in lib.dygnn_last_error()
    hops.id[1] = hops.eid[1] = hops.t[1] = 64
    assert fwd(C.byref(w), dev, 2, 0.1, (64, None), 64, 1 << 40) == -1 and b"null pointer" in lib.dygnn_last_error()
    assert fwd(C.byref(w), dev, 2, 1.0, (64, 64), 64, 1 << 40) == -1 and b"dropout must be in [0, 1)" in lib.dygnn_last_error()
    assert fwd(C.byref(w), dev, 2, -0.5, (64, 64), 64, 1 << 40) == -1
    need = lib.dygnn_cawn_train_workspace_bytes(C.byref(cfg), 2)
    assert fwd(C.byref(w), dev, 2, 0.1, (64, 64), 64, need - 1) == -4 and b"workspace too small" in lib.dygnn_last_error()
    assert fwd(C.byref(w), dev, 2, 0.1, (64, 64), 64, 100) == -4


def test_backward_argument_checks():
    lib = _capi.load()
    cfg = config()
    bwd = lambda w, g, go, B, p, ws, nbytes: lib.dygnn_cawn_backward(C.byref(cfg), w, g, *go, B, p, 7, ws, nbytes, None)
    assert bwd(None, None, (None, None), 0, 0.1, None, 0) == 0
    assert bwd(None, None, (None, None), -3, 0.1, None, 0) == -1
    assert bwd(None, None, (None, None), 2, 0.1, None, 0) == -1 and b"null weights" in lib.dygnn_last_error()
    w = weights()
    assert bwd(C.byref(w), None, (None, None), 2, 0.1, None, 0) == -1 and b"null gradient buffer" in lib.dygnn_last_error()
    g = weights()
    g.feature[1].w_hh = None                                           # the reverse hidden weights' buffer must exist too: it stays zero
    assert bwd(C.byref(w), C.byref(g), (64, 64), 2, 0.1, 64, 1 << 40) == -1 and b"null gradient buffer (an LSTM tensor, direction 1)" in lib.dygnn_last_error()
    g = weights()
    assert bwd(C.byref(w), C.byref(g), (64, None), 2, 0.1, 64, 1 << 40) == -1 and b"null pointer" in lib.dygnn_last_error()
    assert bwd(C.byref(w), C.byref(g), (64, 64), 2, 0.1, None, 1 << 40) == -1 and b"null pointer" in lib.dygnn_last_error()
    assert bwd(C.byref(w), C.byref(g), (64, 64), 2, 1.5, 64, 1 << 40) == -1 and b"dropout must be in [0, 1)" in lib.dygnn_last_error()
    need = lib.dygnn_cawn_train_workspace_bytes(C.byref(cfg), 2)
    assert bwd(C.byref(w), C.byref(g), (64, 64), 2, 0.1, 64, need - 1) == -4 and b"workspace too small" in lib.dygnn_last_error()


def test_enable_training_is_opt_in_and_a_cpu_model_has_no_fallback():
    import torch
    c, cfg, m = make_cpu_model()
    a = (c["src"][:4], c["dst"][:4], c["times"][:4])
    assert m._training_enabled is False                                # off by default: the refusal of test_cawn_cpu.py stands
    m.train()
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=5)
    assert m.enable_training() is m and m._training_enabled is True
    with pytest.raises(_capi.DygnnError, match="no CPU fallback"):     # train mode, recording: past the refusal, stopped by the device check
        m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=5)
    with pytest.raises(NotImplementedError, match="taps are an inference facility"):
        m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=5, taps=2)
    with pytest.raises(NotImplementedError, match="inference-only"):   # the evaluation step has no backward pass in either mode
        m.compute_step_embeddings(a[0], a[1], a[1], a[2], num_neighbors=5)
    m.eval()
    with pytest.raises(NotImplementedError, match="inference-only"):   # eval mode with recording
        m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=5)
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.compute_step_embeddings(a[0], a[1], a[1], a[2], num_neighbors=5)
    with torch.no_grad():
        with pytest.raises(_capi.DygnnError, match="no CPU fallback"):
            m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=5)
    assert m.enable_training(False) is m and m._training_enabled is False
    m.train()
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=5)
