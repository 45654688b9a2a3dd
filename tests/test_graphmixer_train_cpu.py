"""The GraphMixer training entry points without a GPU (ctypes, in the style of test_graphmixer_cpu.py): the exported symbols,
dygnn_graphmixer_train_workspace_bytes and the host-side argument checks of dygnn_graphmixer_train_forward / dygnn_graphmixer_backward, and
the drop-in class's refusal of a CPU model in train mode.  No kernel is launched: every call here fails validation first, or has no roots."""
import ctypes as C
import os

import numpy as np
import pytest

from dyglib_amd import _capi, synthetic as syn
from tests.test_graphmixer_cpu import REFUSED, SUPPORTED, config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dygnn_graphmixer_train_workspace_bytes", "dygnn_graphmixer_train_forward", "dygnn_graphmixer_backward")


def test_symbols_are_exported_and_declared():
    lib = _capi.load()
    header = open(os.path.join(ROOT, "include", "dygnn.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _capi.SIGNATURES and f" {name}(" in header
    assert lib.dygnn_abi_version() == _capi.ABI_VERSION == 21


@pytest.mark.parametrize("kw,rc,msg", REFUSED, ids=[f"{i}" for i in range(len(REFUSED))])
def test_refused_configs(kw, rc, msg):
    lib = _capi.load()
    cfg = config(**kw)
    assert lib.dygnn_graphmixer_train_workspace_bytes(C.byref(cfg), 600) == 0
    assert msg in lib.dygnn_last_error().decode()                            # the inference path's message
    assert lib.dygnn_graphmixer_check(C.byref(cfg)) == rc
    # both entry points refuse the same way before they look at any pointer
    assert lib.dygnn_graphmixer_train_forward(C.byref(cfg), None, None, None, None, None, None, 5, 0.1, 1, None, None, 0, None) == rc
    assert msg in lib.dygnn_last_error().decode()
    assert lib.dygnn_graphmixer_backward(C.byref(cfg), None, None, None, 5, 0.1, 1, None, 0, None) == rc
    assert msg in lib.dygnn_last_error().decode()


@pytest.mark.parametrize("kw", SUPPORTED, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_workspace_bytes_of_supported_configs(kw):
    lib = _capi.load()
    cfg = config(**kw)
    K, Cc, H, L, Ft, Fn = cfg.num_tokens, cfg.edge_feat_dim, cfg.channel_hidden_dim, cfg.num_layers, cfg.time_feat_dim, cfg.node_feat_dim
    last = 0
    for n in (0, 1, 2, 7, 400, 401, 1537):
        b = lib.dygnn_graphmixer_train_workspace_bytes(C.byref(cfg), n)
        assert b > 0 and b >= last, (n, b, last)                                      # positive, non-decreasing in n
        if n > 1:
            assert b > last, (n, b, last)                                             # and it grows with n
        last = b
        assert b > lib.dygnn_graphmixer_workspace_bytes(C.byref(cfg), n), n           # on top of everything the inference forward keeps
        rows = max(n, 1) * K
        # saved: token rows, block inputs, and per block the residual, the LayerNorm output and two hidden arrays
        assert b >= 4 * rows * ((Cc + Ft) + (L + 1) * Cc + L * (2 * Cc + 2 * H)) + 4 * max(n, 1) * (Cc + 2 * Fn)
    big, small = config(**{**kw, "G": 10 ** 9}), config(**{**kw, "G": 1})           # nothing has a time_gap dimension
    assert lib.dygnn_graphmixer_train_workspace_bytes(C.byref(big), 400) == lib.dygnn_graphmixer_train_workspace_bytes(C.byref(small), 400)
    assert lib.dygnn_graphmixer_train_workspace_bytes(C.byref(cfg), -1) == 0 and b"n_roots" in lib.dygnn_last_error()
    assert lib.dygnn_graphmixer_train_workspace_bytes(C.byref(cfg), 2 ** 31) == 0 and b"n_roots" in lib.dygnn_last_error()


def weights(layers=2, time_encoder=True):
    w = _capi.GraphmixerWeights()
    for f, _ in _capi.GraphmixerWeights._fields_:
        if f != "layers" and (time_encoder or not f.startswith("time_")):
            setattr(w, f, 64)
    for l in range(layers):
        for f, _ in _capi.MixerLayerWeights._fields_:
            setattr(w.layers[l], f, 64)
    return w


def csr_of_two_nodes():
    indptr = np.zeros(3, dtype=np.int64)
    return _capi.Csr(2, 0, indptr.ctypes.data, None, None, None), indptr


def test_train_forward_argument_checks():
    lib = _capi.load()
    cfg = config()
    csr, _keep = csr_of_two_nodes()
    fwd = lambda w, g, feats, roots, n, p, out, ws, nbytes: lib.dygnn_graphmixer_train_forward(C.byref(cfg), w, g, *feats, *roots, n, p, 7, out, ws, nbytes, None)
    none2, dev2 = (None, None), (64, 64)
    assert fwd(None, None, none2, none2, 5, 0.1, None, None, 0) == -1 and b"null weights" in lib.dygnn_last_error()
    w = weights(layers=1)
    assert fwd(C.byref(w), None, none2, none2, 5, 0.1, None, None, 0) == -1 and b"null weights (layer 1)" in lib.dygnn_last_error()
    w = weights()
    assert fwd(C.byref(w), None, none2, none2, 5, 0.1, None, None, 0) == -1 and b"bad csr" in lib.dygnn_last_error()
    assert fwd(C.byref(w), C.byref(csr), none2, none2, 5, 0.1, None, None, 0) == -1 and b"bad arguments" in lib.dygnn_last_error()
    assert fwd(C.byref(w), C.byref(csr), dev2, none2, -1, 0.1, None, None, 0) == -1
    assert fwd(C.byref(w), C.byref(csr), dev2, none2, 2 ** 31, 0.1, None, None, 0) == -1 and b"bad arguments" in lib.dygnn_last_error()
    assert fwd(C.byref(w), C.byref(csr), dev2, none2, 0, 0.1, None, None, 0) == 0          # no roots: nothing to do
    assert fwd(C.byref(w), C.byref(csr), dev2, none2, 5, 0.1, None, None, 0) == -1 and b"null pointer" in lib.dygnn_last_error()
    assert fwd(C.byref(w), C.byref(csr), dev2, dev2, 5, 0.1, None, 64, 1 << 40) == -1 and b"null pointer" in lib.dygnn_last_error()
    assert fwd(C.byref(w), C.byref(csr), dev2, dev2, 5, 0.1, 64, None, 1 << 40) == -1 and b"null pointer" in lib.dygnn_last_error()
    assert fwd(C.byref(w), C.byref(csr), dev2, dev2, 5, 1.0, 64, 64, 1 << 40) == -1 and b"dropout must be in [0, 1)" in lib.dygnn_last_error()
    assert fwd(C.byref(w), C.byref(csr), dev2, dev2, 5, -0.5, 64, 64, 1 << 40) == -1
    need = lib.dygnn_graphmixer_train_workspace_bytes(C.byref(cfg), 5)
    assert fwd(C.byref(w), C.byref(csr), dev2, dev2, 5, 0.1, 64, 64, need - 1) == -4 and b"workspace too small" in lib.dygnn_last_error()
    assert fwd(C.byref(w), C.byref(csr), dev2, dev2, 5, 0.1, 64, 64, 100) == -4


def test_backward_argument_checks():
    lib = _capi.load()
    cfg = config()
    bwd = lambda w, g, go, n, p, ws, nbytes: lib.dygnn_graphmixer_backward(C.byref(cfg), w, g, go, n, p, 7, ws, nbytes, None)
    assert bwd(None, None, None, 5, 0.1, None, 0) == -1 and b"null weights" in lib.dygnn_last_error()
    w = weights()
    assert bwd(C.byref(w), None, None, 5, 0.1, None, 0) == -1 and b"null gradient buffer" in lib.dygnn_last_error()
    g = weights(layers=1, time_encoder=False)
    assert bwd(C.byref(w), C.byref(g), 64, 5, 0.1, 64, 1 << 40) == -1 and b"null gradient buffer (layer 1)" in lib.dygnn_last_error()
    g = weights(time_encoder=False)                                          # the frozen time encoder has no gradient buffer
    assert bwd(C.byref(w), C.byref(g), None, -3, 0.1, None, 0) == -1 and b"bad arguments" in lib.dygnn_last_error()
    assert bwd(C.byref(w), C.byref(g), None, 0, 0.1, None, 0) == 0          # no roots: nothing to do
    assert bwd(C.byref(w), C.byref(g), None, 5, 0.1, 64, 1 << 40) == -1 and b"null pointer" in lib.dygnn_last_error()
    assert bwd(C.byref(w), C.byref(g), 64, 5, 0.1, None, 1 << 40) == -1 and b"null pointer" in lib.dygnn_last_error()
    assert bwd(C.byref(w), C.byref(g), 64, 5, 1.5, 64, 1 << 40) == -1 and b"dropout must be in [0, 1)" in lib.dygnn_last_error()
    need = lib.dygnn_graphmixer_train_workspace_bytes(C.byref(cfg), 5)
    assert bwd(C.byref(w), C.byref(g), 64, 5, 0.1, 64, need - 1) == -4 and b"workspace too small" in lib.dygnn_last_error()


def test_cpu_model_in_train_mode_has_no_fallback():
    import torch
    from dyglib_amd import GraphMixer, get_neighbor_sampler
    data, nf, ef = syn.make_bipartite_graph(8, 3, 40, seed=1)
    m = GraphMixer(nf, ef, get_neighbor_sampler(data, "recent", seed=1), 100, num_tokens=10).train()
    a = (data.src_node_ids[:4], data.dst_node_ids[:4], data.node_interact_times[:4])
    assert torch.is_grad_enabled()
    with pytest.raises(_capi.DygnnError, match="no CPU fallback"):
        m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=10, time_gap=5)
    with pytest.raises(_capi.DygnnError, match="no CPU fallback"):
        m.compute_node_temporal_embeddings(a[0], a[2], num_neighbors=10, time_gap=5)
    # what has no backward pass still says so before it looks at the device
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.compute_step_embeddings(a[0], a[1], a[1], a[2], num_neighbors=10, time_gap=5)
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.compute_node_temporal_embeddings(a[0], a[2], num_neighbors=10, time_gap=5, taps=2)
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.eval().compute_src_dst_node_temporal_embeddings(*a, num_neighbors=10, time_gap=5)
    m.train().set_neighbor_sampler(get_neighbor_sampler(data, "uniform", seed=1))
    with pytest.raises(NotImplementedError, match="recent"):
        m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=10, time_gap=5)
