"""GraphMixer without a GPU: the drop-in class's state_dict against the key list the reference recorded in the fixtures, the C structs
against include/dygnn.h, and dygnn_graphmixer_workspace_bytes / dygnn_graphmixer_check / the host-side argument checks of
dygnn_graphmixer_forward (no kernel is launched: every call here fails validation first, or has zero roots)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from dyglib_amd import _build, _capi, synthetic as syn
from tests import golden_cases as gc
from tests import graphmixer_cases as gmc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def config(K=30, G=2000, tokens=None, layers=2, Fn=172, Cc=172, Ft=100, token_hidden=None, channel_hidden=None):
    tokens = K if tokens is None else tokens
    return _capi.GraphmixerConfig(Fn, Cc, Ft, tokens, layers, int(0.5 * tokens) if token_hidden is None else token_hidden,
                                  int(4.0 * Cc) if channel_hidden is None else channel_hidden, K, G, 0)


@pytest.mark.parametrize("name", list(gmc.CASES))
def test_state_dict_matches_the_reference_and_loads_strictly(name):
    import torch
    from dyglib_amd import GraphMixer, get_neighbor_sampler
    r = gmc.CASES[name]
    data, nf, ef = syn.make_bipartite_graph(8, 3, 40, seed=1)
    m = GraphMixer(nf, ef, get_neighbor_sampler(data, "recent", seed=1), gmc.TIME_FEAT_DIM, num_tokens=r["K"], num_layers=r["layers"])
    keys = [str(k) for k in gc.load_golden(f"graphmixer_{name}")["state_dict_keys"]]
    params = syn.make_graphmixer_params(r["param_seed"], r["K"], num_layers=r["layers"])
    assert list(m.state_dict().keys()) == keys == list(params.keys()) and len(keys) == 6 + 12 * r["layers"]
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == syn.graphmixer_param_shapes(r["K"], num_layers=r["layers"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    assert not m.time_encoder.w.weight.requires_grad and not m.time_encoder.w.bias.requires_grad and m.projection_layer.weight.requires_grad
    assert torch.equal(m.mlp_mixers[0].token_norm.weight, torch.from_numpy(params["mlp_mixers.0.token_norm.weight"]))


def test_synthetic_params_would_show_a_dropped_term():
    p = syn.make_graphmixer_params(1, 30)
    for k, v in p.items():
        assert v.dtype == np.float32 and v.flags["C_CONTIGUOUS"], k
        if k.endswith("bias"):
            assert np.abs(v).max() > 1e-3, k
        if "_norm.weight" in k:
            assert np.abs(v - 1).max() > 1e-2, k


def test_struct_layouts_match_header():
    assert C.sizeof(_capi.GraphmixerConfig) == 10 * 4
    assert C.sizeof(_capi.MixerLayerWeights) == 12 * 8
    assert C.sizeof(_capi.GraphmixerWeights) == (4 + 12 * _capi.DYGNN_MAX_LAYERS + 2) * 8
    assert C.sizeof(_capi.GraphmixerTaps) == (1 + 1 + _capi.DYGNN_MAX_LAYERS + 2) * 8
    header = open(os.path.join(ROOT, "include", "dygnn.h")).read()
    body = re.search(r"typedef struct dygnn_graphmixer_config \{(.*?)\} dygnn_graphmixer_config;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.replace("int32_t", "").split(",")]
    assert names == [f[0] for f in _capi.GraphmixerConfig._fields_]
    body = re.search(r"typedef struct dygnn_mixer_layer_weights \{(.*?)\} dygnn_mixer_layer_weights;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\*(\w+)", body) == [f[0] for f in _capi.MixerLayerWeights._fields_]
    assert _capi.load().dygnn_abi_version() == _capi.ABI_VERSION == int(re.search(r"dygnn_abi_version\(void\) \{ return (\d+); \}",
                                                                                 open(os.path.join(_build.CSRC, "csr_host.cpp")).read()).group(1))


SUPPORTED = [dict(K=10), dict(K=20), dict(K=30), dict(K=2), dict(K=3), dict(K=17), dict(K=32), dict(K=30, G=1), dict(K=30, G=10 ** 9),
             dict(K=30, layers=1), dict(K=30, layers=_capi.DYGNN_MAX_LAYERS), dict(K=4, Fn=16, Cc=16, Ft=16), dict(K=4, Fn=32, Cc=32, Ft=16),
             dict(K=4, Fn=16, Cc=32, Ft=16, layers=3)]


@pytest.mark.parametrize("kw", SUPPORTED, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_workspace_bytes_of_supported_configs(kw):
    lib = _capi.load()
    cfg = config(**kw)
    assert lib.dygnn_graphmixer_check(C.byref(cfg)) == 0
    for n in (1, 2, 600, 19200):
        b = lib.dygnn_graphmixer_workspace_bytes(C.byref(cfg), n)
        floats = n * (cfg.num_tokens * cfg.edge_feat_dim + cfg.node_feat_dim)       # the token activations and the node-encoder term: no time_gap
        assert 4 * floats <= b <= 4 * floats + 512, (n, b)
    big, small = config(**{**kw, "G": 10 ** 9}), config(**{**kw, "G": 1})
    assert lib.dygnn_graphmixer_workspace_bytes(C.byref(big), 600) == lib.dygnn_graphmixer_workspace_bytes(C.byref(small), 600)
    assert lib.dygnn_graphmixer_workspace_bytes(C.byref(cfg), 0) > 0


REFUSED = [
    (dict(K=0, tokens=30), -1, "Number of sampled neighbors for each node should be greater than 0!"),
    (dict(K=-3, tokens=30), -1, "Number of sampled neighbors for each node should be greater than 0!"),
    (dict(K=30, G=0), -1, "time_gap must be greater than 0"),
    (dict(K=30, G=-1), -1, "time_gap must be greater than 0"),
    (dict(K=20, tokens=30), -1, "num_neighbors (20) must equal num_tokens (30)"),
    (dict(K=30, layers=0), -1, "num_layers must be at least 1"),
    (dict(K=30, layers=_capi.DYGNN_MAX_LAYERS + 1), -3, f"num_layers {_capi.DYGNN_MAX_LAYERS + 1} > {_capi.DYGNN_MAX_LAYERS} not supported"),
    (dict(K=1), -3, "num_tokens 1 not supported"),
    (dict(K=33), -3, "num_tokens 33 not supported"),
    (dict(K=30, Fn=170), -3, "multiples of 4"),
    (dict(K=30, Cc=260), -3, "feature dims > 256 not supported"),
    (dict(K=30, channel_hidden=100), -3, "channel_hidden_dim 100 not supported"),
    (dict(K=30, token_hidden=0), -3, "token_hidden_dim 0 not supported"),
    (dict(K=30, token_hidden=17), -3, "token_hidden_dim 17 not supported"),
]


@pytest.mark.parametrize("kw,rc,msg", REFUSED, ids=[f"{i}" for i in range(len(REFUSED))])
def test_refused_configs(kw, rc, msg):
    lib = _capi.load()
    cfg = config(**kw)
    assert lib.dygnn_graphmixer_workspace_bytes(C.byref(cfg), 600) == 0
    assert msg in lib.dygnn_last_error().decode()
    assert lib.dygnn_graphmixer_check(C.byref(cfg)) == rc
    # the forward refuses the same way before it looks at any pointer
    assert lib.dygnn_graphmixer_forward(C.byref(cfg), None, None, None, None, None, None, 5, None, None, None, 0, None) == rc
    with pytest.raises(AssertionError if rc == -1 else NotImplementedError):
        _capi.check(rc)


def test_forward_argument_checks():
    lib = _capi.load()
    cfg = config()
    w = _capi.GraphmixerWeights()
    fwd = lambda *a: lib.dygnn_graphmixer_forward(C.byref(cfg), *a)
    assert fwd(None, None, None, None, None, None, 5, None, None, None, 0, None) == -1 and b"null weights" in lib.dygnn_last_error()
    for f, _ in _capi.GraphmixerWeights._fields_:
        if f != "layers":
            setattr(w, f, 64)
    assert fwd(C.byref(w), None, None, None, None, None, 5, None, None, None, 0, None) == -1 and b"null layer weights (layer 0)" in lib.dygnn_last_error()
    for l in range(2):
        for f, _ in _capi.MixerLayerWeights._fields_:
            setattr(w.layers[l], f, 64)
    assert fwd(C.byref(w), None, None, None, None, None, 5, None, None, None, 0, None) == -1 and b"bad csr" in lib.dygnn_last_error()
    indptr = np.zeros(3, dtype=np.int64)
    csr = _capi.Csr(2, 0, indptr.ctypes.data, None, None, None)
    assert fwd(C.byref(w), C.byref(csr), None, None, None, None, 5, None, None, None, 0, None) == -1 and b"bad arguments" in lib.dygnn_last_error()
    assert fwd(C.byref(w), C.byref(csr), 64, 64, None, None, -1, None, None, None, 0, None) == -1
    assert fwd(C.byref(w), C.byref(csr), 64, 64, None, None, 0, None, None, None, 0, None) == 0          # no roots: nothing to do
    assert fwd(C.byref(w), C.byref(csr), 64, 64, None, None, 5, None, None, None, 0, None) == -1 and b"null pointer" in lib.dygnn_last_error()
    assert fwd(C.byref(w), C.byref(csr), 64, 64, 64, 64, 5, 64, None, 64, 100, None) == -4 and b"workspace too small" in lib.dygnn_last_error()


def test_evaluation_loop_still_refuses_other_models_and_graphmixer_is_exported():
    import torch
    import dyglib_amd
    from dyglib_amd import evaluate_model_link_prediction
    assert "GraphMixer" in dyglib_amd.__all__ and dyglib_amd.GraphMixer.__name__ == "GraphMixer"
    for name in ("JODIE", "DyRep", "CAWN", "TCL", "graphmixer"):
        with pytest.raises(ValueError, match="Wrong value for model_name"):
            evaluate_model_link_prediction(name, None, None, [], dyglib_amd.NegativeEdgeSampler(np.arange(3), np.arange(3), seed=0), None, torch.nn.BCELoss())


def test_cpu_model_and_autograd_are_refused_without_a_gpu():
    import torch
    from dyglib_amd import GraphMixer, get_neighbor_sampler
    data, nf, ef = syn.make_bipartite_graph(8, 3, 40, seed=1)
    m = GraphMixer(nf, ef, get_neighbor_sampler(data, "recent", seed=1), 100, num_tokens=10).eval()
    a = (data.src_node_ids[:4], data.dst_node_ids[:4], data.node_interact_times[:4])
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=10, time_gap=5)
    with torch.no_grad(), pytest.raises(_capi.DygnnError, match="no CPU fallback"):
        m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=10, time_gap=5)
    m.set_neighbor_sampler(get_neighbor_sampler(data, "uniform", seed=1))
    with torch.no_grad(), pytest.raises(NotImplementedError, match="recent"):
        m.compute_step_embeddings(a[0], a[1], a[1], a[2], num_neighbors=10, time_gap=5)


# ---- the same host-side validation under AddressSanitizer + UndefinedBehaviorSanitizer (the `asan` library variant, host code only) ----------
@pytest.mark.timeout(900)
def test_host_validation_is_clean_under_asan_ubsan():
    _build.build(verbose=False, variant="asan")
    env = dict(os.environ)
    env.update(LD_PRELOAD=_build.asan_runtime(), DYGNN_LIB_VARIANT="asan", ASAN_OPTIONS="detect_leaks=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_graphmixer_cpu.py", "-m", "not gpu", "-x", "-q", "-p", "no:cacheprovider",
                        "-k", "workspace_bytes or refused or argument_checks or struct_layouts"], cwd=ROOT, env=env, capture_output=True, text=True)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert re.search(r"\d+ passed", out) and "libdygnn_hip_asan.so" in subprocess.run(
        [sys.executable, "-c", "from dyglib_amd import _capi; print(_capi.load()._name)"], cwd=ROOT, env=env, capture_output=True, text=True).stdout
