"""Every backbone with timestamps 10 and 1000 times those of the fixture graphs (tests/large_timestamp_cases.py), against its oracle.

The time encoder's argument fma(dt, w, b) stays below 2.7e6 rad on every fixture graph.  x10 reaches 2.7e7, the top decade of the fast range
reduction of dyglib_amd/csrc/time_encoding.h; x1000 sends the highest frequencies beyond kFastMax = 3e7, so that cos_time makes its
out-of-line call into libm (tgat.hip, tgat_attn.h, tgat_train.hip, tcl.hip, tcl_train.hip, cawn.hip, cawn_train.hip, graphmixer.hip,
graphmixer_train.hip), sin_time its call into sinf (dygformer_train.hip: k_time_bwd), and the message rows of TGN, JODIE and DyRep their cosf
on arguments up to 2.7e9, in waves whose other lanes stay on the fast path.  Each test asserts that its case reaches that range
(lt.require_ranges, on the case's own parameters and sampled time differences).

Inference: embeddings (and the memory bank a run leaves) with `close`, plain 1e-4.  Training at dropout 0: embeddings with `close`, every
parameter gradient with `close_scaled`.  The gradient reference is the float32 autograd oracle, time_encoder.w.weight (whose terms carry dt
up to 2.7e9) included: tests/test_large_timestamps_cpu.py holds each oracle, on these very cases, to a quarter of the close_scaled bar from
its own float64 evaluation behind the float32 argument (observed: below 0.025 of the bar for every tensor)."""
import numpy as np
import pytest
import torch

from tests import large_timestamp_cases as lt
from tests.parity import close, close_scaled

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", params=lt.SCALES, ids=lambda s: f"x{s}")
def base(request):
    return lt.scaled_case(request.param)


def case_of(name, base):
    """the backbone's case on the scaled graph, its range condition asserted"""
    c = lt.CASES[name](base)
    got = lt.require_ranges(base["scale"], c[lt.PARAMS[name]], lt.time_differences(name, c), f"{name} x{base['scale']}")
    print(f"{name} x{base['scale']}: {got}")
    return c, f"large timestamps x{base['scale']}: {name}"


def compare_gradients(tag, got, want, skip=()):
    assert set(want) - set(skip) <= set(got), set(want) - set(got)
    for n, ref in want.items():
        if n not in skip:
            assert got[n] is not None, n
            close_scaled(got[n], ref, f"{tag} grad {n}", label=f"{tag} training gradients vs oracle autograd (scaled bar)")
    if lt.TIME_W in want and lt.TIME_W not in skip:
        close_scaled(got[lt.TIME_W], want[lt.TIME_W], f"{tag} grad {lt.TIME_W}", label=f"{tag} training, time-encoder weight gradient alone (scaled bar)")


def hip_grads(model):
    return {n: (None if p.grad is None else p.grad.detach().cpu().numpy()) for n, p in model.named_parameters()}


# ---- TGAT --------------------------------------------------------------------------------------------------------------------------------------
def test_tgat_inference(base):
    from oracle import tgat_oracle as torc
    from tests.test_tgat import _model
    c, tag = case_of("tgat", base)
    want = torc.tgat_forward(c["tgat_params"], c["node_feat"], c["edge_feat"], c["adj"], c["src"], c["dst"], c["times"], lt.TGAT["L"], lt.TGAT["k"], lt.TGAT["H"])
    with torch.no_grad():
        got = _model(c).compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=lt.TGAT["k"])
    for g, w, side in zip(got, want, ("src", "dst")):
        close(g.cpu().numpy(), w.numpy(), f"{tag} inference {side}", label=f"{tag} inference vs oracle")


def test_tgat_training(base):
    from tests.test_tgat_train_gpu import _model
    c, tag = case_of("tgat", base)
    model = _model(c)
    s, d = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=lt.TGAT["k"])
    lt.pair_loss(s, d).backward()
    want_emb, want = lt.tgat_oracle(c)
    for g, w, side in zip((s, d), want_emb, ("src", "dst")):
        close(g.detach().cpu().numpy(), w, f"{tag} training {side}", label=f"{tag} training embeddings vs oracle")
    compare_gradients(tag, hip_grads(model), want)


# ---- TGN ---------------------------------------------------------------------------------------------------------------------------------------
def test_tgn_inference_over_three_batches(base):
    """negative call, then positive call per batch; the four blocks of every batch, then memory and last-update times"""
    from oracle import tgn_oracle as tn
    from tests.test_tgn_train_gpu import _calls, _model
    c, tag = case_of("tgn", base)
    m = _model(c, train=False)
    P = {k: torch.from_numpy(v) for k, v in c["tgn_params"].items()}
    nf, ef = torch.from_numpy(c["node_feat"]), torch.from_numpy(c["edge_feat"])
    st = tn.TgnState(c["node_feat"].shape[0], 172)
    args = (lt.TGN["L"], lt.TGN["k"], lt.TGN["H"])
    with torch.no_grad():
        for i, b in enumerate(c["tgn_batches"]):
            got = _calls(m, c, b)
            want = tn.tgn_forward(P, nf, ef, c["adj"], st, b["src"], b["neg"], b["t"], None, False, *args)
            want += tn.tgn_forward(P, nf, ef, c["adj"], st, b["src"], b["dst"], b["t"], b["eid"], True, *args)
            for g, w, what in zip(got, want, ("neg src", "neg dst", "pos src", "pos dst")):
                close(g.cpu().numpy(), w.numpy(), f"{tag} batch {i} {what}", label=f"{tag} inference vs oracle")
    assert len(st.last_msg) > 0 and float(st.M.abs().max()) > 0          # the message rows ran and were consumed
    close(m.memory_bank.node_memories.data.cpu().numpy(), st.M.numpy(), f"{tag} memory", label=f"{tag} final memory vs oracle")
    close(m.memory_bank.node_last_updated_times.data.cpu().numpy(), st.U.numpy(), f"{tag} last update", label=f"{tag} final last-update times vs oracle")


def test_tgn_training(base):
    from tests import tgn_autograd as ta
    from tests.test_tgn_train_gpu import _calls, _grads, _model, _replay
    c, tag = case_of("tgn", base)
    model = _model(c)
    _replay(model, c, c["tgn_batches"][:-1])
    assert model.memory_bank.has_msg.any()
    embs = _calls(model, c, c["tgn_batches"][-1])
    ta.step_loss(*embs).backward()
    want_emb, want = lt.tgn_oracle(c)
    for g, w, what in zip(embs, want_emb, ("neg src", "neg dst", "pos src", "pos dst")):
        close(g.detach().cpu().numpy(), w, f"{tag} training {what}", label=f"{tag} training embeddings vs oracle")
    got = _grads(model)
    assert set(got) == set(want)
    compare_gradients(tag, got, want)


# ---- TCL ---------------------------------------------------------------------------------------------------------------------------------------
def _tcl_model(c):
    from tests.test_tcl_gpu import make_model
    return make_model(c["node_feat"], c["edge_feat"], c["data"], c["tcl_params"], lt.TCL["K"], lt.TCL["L"], lt.TCL["H"])


def test_tcl_inference(base):
    from tests import tcl_oracle as tco
    c, tag = case_of("tcl", base)
    m = _tcl_model(c)
    with torch.no_grad():
        got = m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=lt.TCL["K"])
    a, b = (m.neighbor_sampler.get_historical_neighbors(c[side], c["times"], lt.TCL["K"]) for side in ("src", "dst"))
    for mine, ref in zip(list(a) + list(b), [x for side in lt.tcl_neighbours(c) for x in side]):          # the sampler is bit-exact at these times too
        assert np.array_equal(np.asarray(mine), ref)
    want = tco.tcl_forward(c["tcl_params"], c["node_feat"], c["edge_feat"], c["src"], c["dst"], c["times"], a, b, lt.TCL["L"], lt.TCL["H"])
    for g, w, side in zip(got, want, ("src", "dst")):
        close(g.cpu().numpy(), w, f"{tag} inference {side}", label=f"{tag} inference vs oracle")


def test_tcl_training(base):
    c, tag = case_of("tcl", base)
    m = _tcl_model(c).train()
    m.dropout = 0.0
    s, d = m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=lt.TCL["K"])
    lt.pair_loss(s, d).backward()
    want_emb, want = lt.tcl_oracle(c)
    for g, w, side in zip((s, d), want_emb, ("src", "dst")):
        close(g.detach().cpu().numpy(), w, f"{tag} training {side}", label=f"{tag} training embeddings vs oracle")
    compare_gradients(tag, hip_grads(m), want)


# ---- CAWN --------------------------------------------------------------------------------------------------------------------------------------
def test_cawn_inference(base):
    from dyglib_amd import CAWN, get_neighbor_sampler
    from tests import cawn_cases as cc
    from tests import cawn_oracle as cwo
    c, tag = case_of("cawn", base)
    W, k, heads = lt.CAWN["W"], lt.CAWN["k"], lt.CAWN["heads"]
    sampler = get_neighbor_sampler(c["data"], "recent", seed=1, device=DEV)
    m = CAWN(c["node_feat"], c["edge_feat"], sampler, cc.TIME_FEAT_DIM, lt.CAWN["P"], walk_length=W, num_walk_heads=heads, device=DEV)
    m.load_state_dict({n: torch.from_numpy(v) for n, v in c["cawn_params"].items()}, strict=True)
    m = m.to(DEV).eval()
    with torch.no_grad():
        got = m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=k)
    a, b = sampler.get_multi_hop_neighbors(W, c["src"], c["times"], k), sampler.get_multi_hop_neighbors(W, c["dst"], c["times"], k)
    want = cwo.cawn_forward(c["cawn_params"], c["node_feat"], c["edge_feat"], c["src"], c["dst"], c["times"], a, b, heads)
    for g, w, side in zip(got, want, ("src", "dst")):
        close(g.cpu().numpy(), w, f"{tag} inference {side}", label=f"{tag} inference vs oracle")


def test_cawn_training(base):
    from tests import cawn_cases as cc
    from tests.test_cawn_train_gpu import hip_sides_run, make_model
    c, tag = case_of("cawn", base)
    m = make_model(c["data"], c["node_feat"], c["edge_feat"], c["cawn_params"], cc.TIME_FEAT_DIM, lt.CAWN["P"], lt.CAWN["W"], lt.CAWN["heads"]).enable_training()
    s, d, got = hip_sides_run(m, c["sides"], lt.CAWN["k"], (1, 2))
    want_emb, want = lt.cawn_oracle(c)
    for g, w, side in zip((s, d), want_emb, ("src", "dst")):
        close(g, w, f"{tag} training {side}", label=f"{tag} training embeddings vs oracle")
    compare_gradients(tag, got, want)


# ---- GraphMixer --------------------------------------------------------------------------------------------------------------------------------
def _graphmixer_model(c):
    from tests.test_graphmixer_gpu import make_model
    return make_model(c["node_feat"], c["edge_feat"], c["data"], c["gm_params"], lt.GRAPHMIXER["K"], lt.GRAPHMIXER["L"])


def test_graphmixer_inference(base):
    from tests import graphmixer_oracle as gmo
    c, tag = case_of("graphmixer", base)
    K, G, L = lt.GRAPHMIXER["K"], lt.GRAPHMIXER["G"], lt.GRAPHMIXER["L"]
    with torch.no_grad():
        got = _graphmixer_model(c).compute_node_temporal_embeddings(c["nodes"], c["node_times"], num_neighbors=K, time_gap=G)
    want = gmo.graphmixer_forward(c["gm_params"], c["node_feat"], c["edge_feat"], c["adj"], c["nodes"], c["node_times"], K, G, L)
    close(got.cpu().numpy(), want, f"{tag} inference", label=f"{tag} inference vs oracle")


def test_graphmixer_training(base):
    """the time encoder is frozen in GraphMixer: cos_time runs in the training forward, no time-encoder gradient exists"""
    c, tag = case_of("graphmixer", base)
    K, G, n = lt.GRAPHMIXER["K"], lt.GRAPHMIXER["G"], len(c["src"])
    m = _graphmixer_model(c).train()
    m.dropout = 0.0
    emb = m.compute_node_temporal_embeddings(c["nodes"], c["node_times"], num_neighbors=K, time_gap=G)
    lt.pair_loss(emb[:n], emb[n:]).backward()
    want_emb, want = lt.graphmixer_oracle(c)
    close(emb.detach().cpu().numpy(), np.concatenate(want_emb), f"{tag} training", label=f"{tag} training embeddings vs oracle")
    got = hip_grads(m)
    assert got[lt.TIME_W] is None and got[lt.TIME_B] is None and lt.TIME_W not in want
    compare_gradients(tag, got, want)


# ---- JODIE, DyRep ------------------------------------------------------------------------------------------------------------------------------
def test_jodie_inference_over_three_batches(base):
    from tests.test_memory_variants_gpu import _against_oracle, _model
    c, tag = case_of("jodie", base)
    pend = _against_oracle(_model(c["node_feat"], c["edge_feat"], c["params"], c["shifts"]), c["params"], c["edge_feat"], c["shifts"], c["batches"], tag)
    assert pend[0] == 0 and pend[-1] > 0                                 # fresh bank (dt = t - 0), then pending messages


def test_dyrep_inference_over_three_batches(base):
    from tests.test_memory_variants_gpu import _dyrep_against_oracle
    c, tag = case_of("dyrep", base)
    pend = _dyrep_against_oracle(c, c["batches"], tag)
    assert pend[0] == 0 and pend[-1] > 0


# ---- DyGFormer ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", [1, 3])
def test_dygformer_inference_in_the_top_decade(impl):
    """x10 only: x1000 is tests/test_dygformer_gpu.py::test_large_timestamps_take_the_libm_cosine_path"""
    from tests.test_dygformer_gpu import build_model
    c, tag = case_of("dygformer", lt.scaled_case(10))
    cfg = c["cfg"]
    model, _ = build_model(c)
    model.impl = impl
    with torch.no_grad():
        want = lt.orc.dygformer_forward(c["params"], c["node_feat"], c["edge_feat"], c["adj"], c["src"], c["dst"], c["times"], cfg["patch_size"],
                                        cfg["max_input_sequence_length"])
        got = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"])
    for g, w, side in zip(got, want, ("src", "dst")):
        close(g.cpu().numpy(), w.numpy(), f"{tag} impl {impl} inference {side}", label=f"{tag} impl {impl} inference vs oracle")


@pytest.mark.parametrize("path", ["fused", "product-by-product"])
def test_dygformer_training(base, path, monkeypatch):
    """both training paths; at x1000 the time encoder's gradient takes sin_time through sinf (dygformer_train.hip: k_time_bwd)"""
    from tests.test_dygformer_gpu import build_model
    if path != "fused":
        monkeypatch.setenv("DYGNN_TRAIN_UNFUSED", "1")
    c, tag = case_of("dygformer", base)
    tag += f" ({path})"
    model, _ = build_model(c)
    model.eval()                                                         # dropout off, autograd on: the training kernels with p = 0
    s, d = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"])
    assert s.requires_grad and d.requires_grad
    lt.pair_loss(s, d).backward()
    want_emb, want = lt.dygformer_oracle(c)
    for g, w, side in zip((s, d), want_emb, ("src", "dst")):
        close(g.detach().cpu().numpy(), w, f"{tag} training {side}", label=f"{tag} training embeddings vs oracle")
    compare_gradients(tag, hip_grads(model), want)
