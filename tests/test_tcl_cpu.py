"""TCL without a GPU: the drop-in class's state_dict against the key list the reference recorded in the fixtures, the C structs against
include/dygnn.h, and dygnn_tcl_check / dygnn_tcl_workspace_bytes / the host-side argument checks of dygnn_tcl_forward (no kernel is launched:
every call here fails validation first, or has zero pairs)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dyglib_amd import _capi, synthetic as syn
from tests import golden_cases as gc
from tests import tcl_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def config(K=20, layers=2, heads=2, Fn=172, Fe=172, Ft=100, node_rows=50, edge_rows=50):
    return _capi.TclConfig(Fn, Fe, Ft, K, layers, heads, node_rows, edge_rows)


@pytest.mark.parametrize("name", list(tc.CASES))
def test_state_dict_matches_the_reference_and_loads_strictly(name):
    import torch
    import dyglib_amd
    from dyglib_amd import TCL, get_neighbor_sampler
    assert "TCL" in dyglib_amd.__all__ and TCL.__name__ == "TCL"
    r = tc.CASES[name]
    data, nf, ef = syn.make_bipartite_graph(8, 3, 40, seed=1)
    m = TCL(nf, ef, get_neighbor_sampler(data, "recent", seed=1), tc.TIME_FEAT_DIM, num_layers=r["layers"], num_heads=r["heads"], num_depths=r["K"] + 1)
    keys = [str(k) for k in gc.load_golden(f"tcl_{name}")["state_dict_keys"]]
    params = syn.make_tcl_params(r["param_seed"], r["K"], num_layers=r["layers"])
    assert list(m.state_dict().keys()) == keys == list(params.keys()) and len(keys) == 11 + 12 * r["layers"]
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == syn.tcl_param_shapes(r["K"], num_layers=r["layers"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    assert m.time_encoder.w.weight.requires_grad and m.num_depths == r["K"] + 1 and m.num_heads == r["heads"]
    assert torch.equal(m.transformers[0].multi_head_attention.in_proj_bias, torch.from_numpy(params["transformers.0.multi_head_attention.in_proj_bias"]))


def test_synthetic_params_would_show_a_dropped_term():
    p = syn.make_tcl_params(1, 20)
    for k, v in p.items():
        assert v.dtype == np.float32 and v.flags["C_CONTIGUOUS"], k
        if k.endswith("bias"):
            assert np.abs(v).max() > 1e-3, k
        if "norm_layers" in k and k.endswith("weight"):
            assert np.abs(v - 1).max() > 1e-2, k
    assert np.abs(p["depth_embedding.weight"]).max() > 0.5


def test_struct_layouts_match_header():
    assert C.sizeof(_capi.TclConfig) == 8 * 4
    assert C.sizeof(_capi.TclLayerWeights) == 12 * 8
    assert C.sizeof(_capi.TclWeights) == (9 + 12 * _capi.DYGNN_MAX_LAYERS + 2) * 8
    assert C.sizeof(_capi.TclTaps) == (2 + _capi.DYGNN_MAX_LAYERS) * 8
    header = open(os.path.join(ROOT, "include", "dygnn.h")).read()
    strip = lambda body: re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    body = strip(re.search(r"typedef struct dygnn_tcl_config \{(.*?)\} dygnn_tcl_config;", header, re.S).group(1))
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.replace("int32_t", "").split(",")]
    assert names == [f[0] for f in _capi.TclConfig._fields_]
    body = strip(re.search(r"typedef struct dygnn_tcl_layer_weights \{(.*?)\} dygnn_tcl_layer_weights;", header, re.S).group(1))
    assert re.findall(r"\*(\w+)", body) == [f[0] for f in _capi.TclLayerWeights._fields_]
    body = strip(re.search(r"typedef struct dygnn_tcl_weights \{(.*?)\} dygnn_tcl_weights;", header, re.S).group(1))
    assert re.findall(r"\*(\w+)", body) == [f[0] for f in _capi.TclWeights._fields_ if f[0] != "layers"]


SUPPORTED = [dict(K=1), dict(K=5), dict(K=20), dict(K=63), dict(heads=1), dict(heads=4), dict(K=10, layers=1),
             dict(layers=_capi.DYGNN_MAX_LAYERS), dict(K=4, Fn=16, Fe=16, Ft=16, heads=8), dict(K=4, Fn=32, Fe=16, Ft=16), dict(Fn=256, Fe=256, Ft=256, heads=8)]


@pytest.mark.parametrize("kw", SUPPORTED, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_workspace_bytes_of_supported_configs(kw):
    lib = _capi.load()
    cfg = config(**kw)
    assert lib.dygnn_tcl_check(C.byref(cfg)) == 0
    seq = 4 * (cfg.num_neighbors + 1) * cfg.node_feat_dim
    for n, p in ((2, 1), (600, 400), (800, 400), (3, 1537)):
        b = lib.dygnn_tcl_workspace_bytes(C.byref(cfg), n, p)
        m = max(n, 2 * p)
        want = (2 * n + 4 * m + 4 * p) * seq + 16 * p       # sides twice, Q K V O, the pairs' sequences twice, the pair index
        assert want <= b <= want + 8 * 256, (n, p, b, want)
    assert lib.dygnn_tcl_workspace_bytes(C.byref(cfg), 0, 0) > 0
    assert lib.dygnn_tcl_workspace_bytes(C.byref(cfg), -1, 1) == 0 and lib.dygnn_tcl_workspace_bytes(C.byref(cfg), 1, -1) == 0


REFUSED = [
    (dict(K=0), -1, "Number of sampled neighbors for each node should be greater than 0!"),
    (dict(K=-2), -1, "Number of sampled neighbors for each node should be greater than 0!"),
    (dict(layers=0), -1, "num_layers and num_heads must be at least 1"),
    (dict(heads=0), -1, "num_layers and num_heads must be at least 1"),
    (dict(K=64), -3, "num_neighbors 64 not supported (1..63)"),
    (dict(Fn=170, heads=1), -3, "must be multiples of 4 (170, 172, 100)"),
    (dict(Fe=6), -3, "must be multiples of 4 (172, 6, 100)"),
    (dict(Ft=50), -3, "must be multiples of 4 (172, 172, 50)"),
    (dict(Fn=260), -3, "node_feat_dim 260 > 256 not supported"),
    (dict(Fe=260), -3, "edge_feat_dim 260 > 256 not supported"),
    (dict(Ft=260), -3, "time_feat_dim 260 > 256 not supported"),
    (dict(heads=3), -3, "num_heads 3 does not divide node_feat_dim 172"),
    (dict(Fn=144, heads=9), -3, "num_heads 9 > 8 not supported"),
    (dict(layers=_capi.DYGNN_MAX_LAYERS + 1), -3, f"num_layers {_capi.DYGNN_MAX_LAYERS + 1} > {_capi.DYGNN_MAX_LAYERS} not supported"),
]


@pytest.mark.parametrize("kw,rc,msg", REFUSED, ids=[f"{i}" for i in range(len(REFUSED))])
def test_refused_configs(kw, rc, msg):
    lib = _capi.load()
    cfg = config(**kw)
    assert lib.dygnn_tcl_workspace_bytes(C.byref(cfg), 600, 400) == 0
    assert msg in lib.dygnn_last_error().decode()
    assert lib.dygnn_tcl_check(C.byref(cfg)) == rc
    # the forward refuses the same way before it looks at any pointer
    assert lib.dygnn_tcl_forward(C.byref(cfg), None, None, None, None, None, None, None, None, 5, None, None, 5, None, None, None, None, 0, None) == rc
    assert msg in lib.dygnn_last_error().decode()
    with pytest.raises(AssertionError if rc == -1 else NotImplementedError):
        _capi.check(rc)


def test_forward_argument_checks():
    lib = _capi.load()
    cfg = config()
    fwd = lambda *a: lib.dygnn_tcl_forward(C.byref(cfg), *a)
    nothing = (None,) * 7
    assert fwd(None, *nothing, 5, None, None, 0, None, None, None, None, 0, None) == 0                   # no pairs: nothing to do
    assert fwd(None, *nothing, 5, None, None, -1, None, None, None, None, 0, None) == -1
    assert fwd(None, *nothing, 5, None, None, 2, None, None, None, None, 0, None) == -1 and b"null weights" in lib.dygnn_last_error()
    w = _capi.TclWeights()
    for f, _ in _capi.TclWeights._fields_:
        if f != "layers":
            setattr(w, f, 64)
    assert fwd(C.byref(w), *nothing, 5, None, None, 2, None, None, None, None, 0, None) == -1 and b"null layer weights (layer 0)" in lib.dygnn_last_error()
    for l in range(2):
        for f, _ in _capi.TclLayerWeights._fields_:
            setattr(w.layers[l], f, 64)
    assert fwd(C.byref(w), *nothing, 5, None, None, 2, None, None, None, None, 0, None) == -1 and b"null pointer" in lib.dygnn_last_error()
    dev = (64,) * 7
    a, b = np.array([0, 4], dtype=np.int32), np.array([1, 5], dtype=np.int32)
    assert fwd(C.byref(w), *dev, 5, a.ctypes.data, b.ctypes.data, 2, 64, 64, None, 64, 1 << 40, None) == -1
    assert b"pair 1 names a side outside [0, 5)" in lib.dygnn_last_error()
    a[1], b[1] = -1, 2
    assert fwd(C.byref(w), *dev, 5, a.ctypes.data, b.ctypes.data, 2, 64, 64, None, 64, 1 << 40, None) == -1
    a[1] = 4
    assert fwd(C.byref(w), *dev, 5, a.ctypes.data, b.ctypes.data, 2, 64, 64, None, 64, 100, None) == -4 and b"workspace too small" in lib.dygnn_last_error()
    assert fwd(C.byref(w), *dev, 5, a.ctypes.data, b.ctypes.data, 2, 64, None, None, 64, 1 << 40, None) == -1 and b"null pointer" in lib.dygnn_last_error()


def test_cpu_model_autograd_and_bad_arguments_are_refused_without_a_gpu():
    import torch
    from dyglib_amd import TCL, get_neighbor_sampler
    data, nf, ef = syn.make_bipartite_graph(8, 3, 40, seed=1)
    m = TCL(nf, ef, get_neighbor_sampler(data, "recent", seed=1), 100, num_depths=11).eval()
    a = (data.src_node_ids[:4], data.dst_node_ids[:4], data.node_interact_times[:4])
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=10)
    m.train()
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.compute_step_embeddings(a[0], a[1], a[1], a[2], num_neighbors=10)
    m.eval()
    with torch.no_grad():
        with pytest.raises(_capi.DygnnError, match="no CPU fallback"):
            m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=10)
        with pytest.raises(_capi.DygnnError, match="no CPU fallback"):
            m.compute_step_embeddings(a[0], a[1], a[1], a[2], num_neighbors=10)
        with pytest.raises(AssertionError, match="num_depths"):
            m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=20)
        with pytest.raises(AssertionError, match="greater than 0"):
            m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=0)
