"""CAWN without a GPU: the CPU restatement tests/cawn_oracle.py against the reference's own outputs (tests/golden/cawn_<case>.npz, written by
tools/make_golden_cawn.py), which also proves its two rewrites (the reverse direction as one cell, step 0 once per side); the drop-in class's
state_dict against the key list the reference recorded; the C structs against include/dygnn.h; dygnn_cawn_check /
dygnn_cawn_workspace_bytes / the host-side argument checks of dygnn_cawn_forward (no kernel is launched: every call here fails validation
first, or has zero pairs); and every refusal of the class on a CPU model.

Tolerances: the project's standing 1e-4 absolute (tests.parity.close) on embeddings and float taps; walk ids exact; position counts 1e-5:
the reference adds 1 / k^h in float32 up to k^h <= 128 times for a sum <= 1, which is within 128 * 2^-24 = 7.7e-6 of count / k^h."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dyglib_amd import _capi, synthetic as syn
from tests import cawn_cases as cc
from tests import cawn_oracle as cwo
from tests import golden_cases as gc
from tests import parity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_TOL = 1e-5
EMB_KEYS = ("src_emb", "dst_emb", "src_neg_emb", "neg_dst_emb")


def check_taps(name, taps, g, what):
    """walk ids exact, counts to COUNT_TOL, encoder / transformer taps at 1e-4"""
    assert np.array_equal(np.asarray(taps["walk_ids"]), g["tap_walk_ids"]), f"{name} walk ids"
    err = float(np.abs(np.asarray(taps["counts"], dtype=np.float64) - g["tap_counts"]).max())
    print(f"{name} {what} counts: max abs err {err:.3e}")
    assert err <= COUNT_TOL, f"{name} counts: max abs err {err:.3e} > {COUNT_TOL:.0e}"
    for key in ("feature_out", "position_out", "attn_in", "attn_out"):
        parity.close(np.asarray(taps[key]), g["tap_" + key], f"{name} {key}", f"{what} {key}")


def oracle_call(c, smp, src, dst, times, taps=False):
    cfg = c["cawn_cfg"]
    a = smp.multi_hop(cfg["W"], src, times, cfg["k"])                # all hops of the sources, then of the destinations (models/CAWN.py:58-64)
    b = smp.multi_hop(cfg["W"], dst, times, cfg["k"])
    return cwo.cawn_forward(c["cawn_params"], c["node_feat"], c["edge_feat"], src, dst, times, a, b, cfg["heads"], taps=taps)


@pytest.mark.parametrize("name", list(cc.CASES))
def test_restatement_matches_reference(name):
    c = cc.build_cawn_case(name)
    g = gc.load_golden(f"cawn_{name}")
    cfg = c["cawn_cfg"]
    smp = cwo.OracleSampler(c["data"], cfg["strategy"], cfg["sampler_seed"], cfg["scale"])
    got = oracle_call(c, smp, c["src"], c["dst"], c["times"]) + oracle_call(c, smp, c["src"], c["neg_dst"], c["times"])
    for x, key in zip(got, EMB_KEYS):
        parity.close(x, g[key], f"{name} {key}", "cawn oracle embeddings")
    r = min(cc.TAP_ROWS, len(c["src"]))
    smp.reset()
    _, _, taps = oracle_call(c, smp, c["src"][:r], c["dst"][:r], c["times"][:r], taps=True)
    check_taps(name, taps, g, "cawn oracle")


def test_fixture_recipes_exercise_what_they_claim():
    sizes = {"gen_w1_k5": (37, 5), "bip_w1_k32": (16, 32), "hub_w2_k4": (12, 16), "gen_w2_k3_uniform": (9, 9)}
    for name, (B, M) in sizes.items():
        c, g = cc.build_cawn_case(name), gc.load_golden(f"cawn_{name}")
        cfg = c["cawn_cfg"]
        assert len(c["src"]) == B and cfg["k"] ** cfg["W"] == M and g["src_emb"].shape == (B, 172) and c["src"].min() > 0
        assert np.abs(g["src_emb"] - g["src_neg_emb"]).max() > 0.02                      # the source embedding depends on its partner
        lens = (g["tap_walk_ids"] != 0).sum(-1)
        assert lens.min() == 1 and lens.max() == cfg["W"] + 1                            # walks of length 1 beside full ones
        both = (g["tap_counts"][..., 0, :].sum(-1) > 0) & (g["tap_counts"][..., 1, :].sum(-1) > 0)
        assert both.any(), name                                                          # a node of both trees
        D = 172 + 172 + cc.TIME_FEAT_DIM + cfg["P"]
        assert g["tap_feature_out"].shape == (cc.TAP_ROWS, 2, M, D) and g["tap_attn_in"].shape[-1] == syn.cawn_attention_dim(D, cfg["heads"])
    c = cc.build_cawn_case("gen_w1_k5")
    assert ((c["hist_src"] == 0) & (c["hist_dst"] == 0)).any() and c["one_sided"] is not None
    assert cc.build_cawn_case("hub_w2_k4")["one_sided"] is not None
    g = gc.load_golden("cawn_hub_w2_k4")
    assert ((g["tap_walk_ids"][..., 1] != 0) & (g["tap_walk_ids"][..., 2] == 0)).any()       # partial walks [t, x, 0]
    assert g["tap_attn_in"].shape[-1] == 236 and gc.load_golden("cawn_bip_w1_k32")["tap_attn_in"].shape[-1] == 312


def make_cpu_model(name="gen_w1_k5"):
    from dyglib_amd import CAWN, get_neighbor_sampler
    c = cc.build_cawn_case(name)
    cfg = c["cawn_cfg"]
    m = CAWN(c["node_feat"], c["edge_feat"], get_neighbor_sampler(c["data"], cfg["strategy"], time_scaling_factor=cfg["scale"], seed=cfg["sampler_seed"]),
             cc.TIME_FEAT_DIM, cfg["P"], walk_length=cfg["W"], num_walk_heads=cfg["heads"])
    return c, cfg, m


@pytest.mark.parametrize("name", list(cc.CASES))
def test_state_dict_matches_the_reference_and_loads_strictly(name):
    import torch
    import dyglib_amd
    assert "CAWN" in dyglib_amd.__all__ and dyglib_amd.CAWN.__name__ == "CAWN"
    c, cfg, m = make_cpu_model(name)
    keys = [str(k) for k in gc.load_golden(f"cawn_{name}")["state_dict_keys"]]
    params = c["cawn_params"]
    assert list(m.state_dict().keys()) == keys == list(params.keys()) and len(keys) == 38
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == syn.cawn_param_shapes(cfg["P"], cfg["W"], cfg["heads"])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, torch.from_numpy(params[k])), k
    assert m.walk_length == cfg["W"] and m.num_walk_heads == cfg["heads"] and m.position_feat_dim == cfg["P"] and m.dropout == 0.1
    assert m.walk_encoder.attention_dim == syn.cawn_attention_dim(444 + cfg["P"], cfg["heads"])
    assert m.walk_encoder.feature_encoder.model_dim == 444 + cfg["P"] and m.position_encoder.walk_length == cfg["W"]


def test_set_neighbor_sampler_resets_a_random_sampler():
    c, cfg, m = make_cpu_model("gen_w2_k3_uniform")
    smp = m.neighbor_sampler
    first = smp.random_state.randint(1 << 30)
    m.set_neighbor_sampler(smp)
    assert m.neighbor_sampler is smp and smp.random_state.randint(1 << 30) == first
    smp.seed = None
    with pytest.raises(AssertionError):
        m.set_neighbor_sampler(smp)


def test_cpu_model_autograd_and_bad_arguments_are_refused_without_a_gpu():
    import torch
    from dyglib_amd import CAWN
    c, cfg, m = make_cpu_model()
    m.eval()
    a = (c["src"][:4], c["dst"][:4], c["times"][:4])
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=5)
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.compute_step_embeddings(a[0], a[1], a[1], a[2], num_neighbors=5)
    m.train()
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=5)
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.compute_step_embeddings(a[0], a[1], a[1], a[2], num_neighbors=5)
    for mode in (m.eval, m.train):
        mode()
        with torch.no_grad():
            with pytest.raises(_capi.DygnnError, match="no CPU fallback"):
                m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=5)
            with pytest.raises(_capi.DygnnError, match="no CPU fallback"):
                m.compute_step_embeddings(a[0], a[1], a[1], a[2], num_neighbors=5)
    with torch.no_grad():
        with pytest.raises(IndexError):
            m.compute_src_dst_node_temporal_embeddings(np.array([10 ** 6]), np.array([1]), np.array([1.0]), num_neighbors=5)
        with pytest.raises(IndexError):
            m.compute_step_embeddings(np.array([1]), np.array([1]), np.array([10 ** 6]), np.array([1.0]), num_neighbors=5)
        with pytest.raises(AssertionError, match="padding node"):
            m.compute_src_dst_node_temporal_embeddings(np.array([1]), np.array([0]), np.array([1.0]), num_neighbors=5)
        with pytest.raises(AssertionError, match="greater than 0"):
            m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=0)
        with pytest.raises(NotImplementedError, match=r"129 walks \(num_neighbors 129 \*\* walk_length 1\) > 128"):
            m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=129)
        deep = CAWN(c["node_feat"], c["edge_feat"], m.neighbor_sampler, cc.TIME_FEAT_DIM, 24, walk_length=3, num_walk_heads=4).eval()
        with pytest.raises(NotImplementedError, match="walk_length 3 not supported"):
            deep.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=2)


def config(Fn=172, Fe=172, Ft=100, P=172, W=1, k=32, heads=8, node_rows=50, edge_rows=50):
    return _capi.CawnConfig(Fn, Fe, Ft, P, W, k, heads, node_rows, edge_rows)


def test_struct_layouts_match_header():
    assert C.sizeof(_capi.CawnConfig) == 9 * 4
    assert C.sizeof(_capi.CawnLstmWeights) == 4 * 8
    assert C.sizeof(_capi.CawnWeights) == (6 + 4 * 4 + 12 + 4) * 8
    assert C.sizeof(_capi.CawnHops) == 6 * 8 and C.sizeof(_capi.CawnTaps) == 7 * 8
    header = open(os.path.join(ROOT, "include", "dygnn.h")).read()
    strip = lambda body: re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    body = strip(re.search(r"typedef struct dygnn_cawn_config \{(.*?)\} dygnn_cawn_config;", header, re.S).group(1))
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.replace("int32_t", "").split(",")]
    assert names == [f[0] for f in _capi.CawnConfig._fields_]
    body = strip(re.search(r"typedef struct dygnn_cawn_lstm_weights \{(.*?)\} dygnn_cawn_lstm_weights;", header, re.S).group(1))
    assert re.findall(r"\*(\w+)", body) == [f[0] for f in _capi.CawnLstmWeights._fields_]
    body = strip(re.search(r"typedef struct dygnn_cawn_weights \{(.*?)\} dygnn_cawn_weights;", header, re.S).group(1))
    assert re.findall(r"(?:\*|weights )(\w+)", body) == [f[0] for f in _capi.CawnWeights._fields_]
    body = strip(re.search(r"typedef struct dygnn_cawn_taps \{(.*?)\} dygnn_cawn_taps;", header, re.S).group(1))
    assert re.findall(r"[ *](\w+);", body) == [f[0] for f in _capi.CawnTaps._fields_]
    lib = _capi.load()
    for name in ("dygnn_cawn_check", "dygnn_cawn_workspace_bytes", "dygnn_cawn_forward"):
        assert hasattr(lib, name) and name in _capi.SIGNATURES and f" {name}(" in header


SUPPORTED = [dict(), dict(k=5), dict(k=1), dict(k=128), dict(W=2, k=4, P=24, heads=4), dict(W=2, k=3), dict(W=2, k=11), dict(Ft=84, heads=5),
             dict(Fn=256, Fe=256, Ft=256, P=256), dict(Fn=16, Fe=16, Ft=16, P=16, heads=2), dict(Fn=32, Fe=16, Ft=16, P=8, heads=1), dict(P=170), dict(W=2, k=3, P=6, heads=4)]


@pytest.mark.parametrize("kw", SUPPORTED, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()) or "wikipedia")
def test_workspace_bytes_of_supported_configs(kw):
    lib = _capi.load()
    cfg = config(**kw)
    assert lib.dygnn_cawn_check(C.byref(cfg)) == 0, lib.dygnn_last_error()
    D = cfg.node_feat_dim + cfg.edge_feat_dim + cfg.time_feat_dim + cfg.position_feat_dim
    A, M = syn.cawn_attention_dim(D, cfg.num_walk_heads), cfg.num_neighbors ** cfg.walk_length
    for n, p in ((2, 1), (600, 400), (3, 1537)):
        b = lib.dygnn_cawn_workspace_bytes(C.byref(cfg), n, p)
        walks = 2 * p * M
        want = 4 * walks * (D + cfg.position_feat_dim + 6 * A)       # the two encoder outputs, X, Q K V, O, Y of every walk
        assert want <= b, (n, p, b, want)
        assert b <= want + 4 * 2 * p * (4 * (1 + cfg.num_neighbors) + 3 * (1 + cfg.num_neighbors + M)) * (D + cfg.position_feat_dim) + 64 * 256
    assert lib.dygnn_cawn_workspace_bytes(C.byref(cfg), 0, 0) > 0
    assert lib.dygnn_cawn_workspace_bytes(C.byref(cfg), -1, 1) == 0 and lib.dygnn_cawn_workspace_bytes(C.byref(cfg), 1, -1) == 0


REFUSED = [
    (dict(k=0), -1, "Number of sampled neighbors for each node should be greater than 0!"),
    (dict(W=0), -1, "Number of sampled hops should be greater than 0!"),
    (dict(heads=0), -1, "num_walk_heads must be at least 1"),
    (dict(W=3, k=2), -3, "walk_length 3 not supported (1..2)"),
    (dict(k=129), -3, "129 walks (num_neighbors 129 ** walk_length 1) > 128 not supported"),
    (dict(W=2, k=12), -3, "144 walks (num_neighbors 12 ** walk_length 2) > 128 not supported"),
    (dict(Fn=260), -3, "node_feat_dim 260 > 256 not supported"),
    (dict(Fe=260), -3, "edge_feat_dim 260 > 256 not supported"),
    (dict(Ft=260), -3, "time_feat_dim 260 > 256 not supported"),
    (dict(P=260), -3, "position_feat_dim 260 > 256 not supported"),
    (dict(Fn=170), -3, "must be multiples of 4 (170, 172, 100)"),
    (dict(Ft=50), -3, "must be multiples of 4 (172, 172, 50)"),
    (dict(P=173), -3, "position_feat_dim 173 is odd"),                          # every odd D has an odd P
    (dict(heads=3), -3, "attention_dim 309 (input dim 616 // 2 rounded up to num_walk_heads 3) is not a multiple of 4"),
    (dict(Fn=256, Fe=256, Ft=256, P=256, heads=12), -3, "attention_dim 516 (input dim 1024 // 2 rounded up to num_walk_heads 12) > 512 not supported"),
    (dict(heads=4), -3, "head size 77 (attention_dim 308 / num_walk_heads 4) > 64 not supported"),
    (dict(heads=2), -3, "head size 154 (attention_dim 308 / num_walk_heads 2) > 64 not supported"),
]


@pytest.mark.parametrize("kw,rc,msg", REFUSED, ids=[f"{i}" for i in range(len(REFUSED))])
def test_refused_configs(kw, rc, msg):
    lib = _capi.load()
    cfg = config(**kw)
    assert lib.dygnn_cawn_workspace_bytes(C.byref(cfg), 600, 400) == 0
    assert msg in lib.dygnn_last_error().decode()
    assert lib.dygnn_cawn_check(C.byref(cfg)) == rc
    # the forward refuses the same way before it looks at any pointer
    assert lib.dygnn_cawn_forward(C.byref(cfg), None, None, None, None, None, None, 5, None, None, 5, None, None, None, None, 0, None) == rc
    assert msg in lib.dygnn_last_error().decode()
    with pytest.raises(AssertionError if rc == -1 else NotImplementedError):
        _capi.check(rc)


def test_forward_argument_checks():
    lib = _capi.load()
    cfg = config(W=2, k=4, P=24, heads=4)
    fwd = lambda *a: lib.dygnn_cawn_forward(C.byref(cfg), *a)
    nothing = (None,) * 5
    assert fwd(None, *nothing, 5, None, None, 0, None, None, None, None, 0, None) == 0                   # no pairs: nothing to do
    assert fwd(None, *nothing, 5, None, None, -1, None, None, None, None, 0, None) == -1
    assert fwd(None, *nothing, 5, None, None, 2, None, None, None, None, 0, None) == -1 and b"null weights" in lib.dygnn_last_error()
    w = _capi.CawnWeights()
    for f, t in _capi.CawnWeights._fields_:
        if t is C.c_void_p:
            setattr(w, f, 64)
    assert fwd(C.byref(w), *nothing, 5, None, None, 2, None, None, None, None, 0, None) == -1
    assert b"null LSTM weights (feature encoder, direction 0)" in lib.dygnn_last_error()
    for enc in (w.feature, w.position):
        for d in range(2):
            for f, _ in _capi.CawnLstmWeights._fields_:
                setattr(enc[d], f, 64)
    assert fwd(C.byref(w), *nothing, 5, None, None, 2, None, None, None, None, 0, None) == -1 and b"null transformer weights" in lib.dygnn_last_error()
    for f, _ in _capi.TclLayerWeights._fields_:
        setattr(w.attn, f, 64)
    assert fwd(C.byref(w), *nothing, 5, None, None, 2, None, None, None, None, 0, None) == -1 and b"null pointer" in lib.dygnn_last_error()
    hops = _capi.CawnHops()
    hops.id[0] = hops.eid[0] = hops.t[0] = 64
    dev = (64, 64, 64, 64, C.byref(hops))
    a, b = np.array([0, 4], dtype=np.int32), np.array([1, 5], dtype=np.int32)
    args = lambda ws: (C.byref(w), *dev, 5, a.ctypes.data, b.ctypes.data, 2, 64, 64, None, 64, ws, None)
    assert fwd(*args(1 << 40)) == -1 and b"null pointer (hop 2 arrays)" in lib.dygnn_last_error()
    hops.id[1] = hops.eid[1] = hops.t[1] = 64
    assert fwd(*args(1 << 40)) == -1 and b"pair 1 names a side outside [0, 5)" in lib.dygnn_last_error()
    a[1], b[1] = -1, 2
    assert fwd(*args(1 << 40)) == -1
    a[1] = 4
    assert fwd(*args(100)) == -4 and b"workspace too small" in lib.dygnn_last_error()
    assert fwd(C.byref(w), *dev, 5, a.ctypes.data, b.ctypes.data, 2, 64, None, None, 64, 1 << 40, None) == -1 and b"null pointer" in lib.dygnn_last_error()
