"""dyglib_amd.JODIE and dyglib_amd.DyRep without a GPU: the oracle (tests/memory_variant_oracle.py) against the reference's own outputs
(tests/golden/jodie_<case>.npz, dyrep_<case>.npz; tools/make_golden_memory_variants.py), the modules' state_dicts, constructors and refusals, the
vectorised compute_src_dst_node_time_shifts, the argument checks of both models' C ABI, and what the recipes must cover.  No kernel is launched here."""
import ctypes as C

import numpy as np
import pytest
import torch

import dyglib_amd
from dyglib_amd import _capi, synthetic as syn
from tests import golden_cases as gc
from tests import memory_variant_cases as mv
from tests import memory_variant_oracle as mo
from tests.parity import close  # plain 1e-4 absolute


@pytest.fixture(scope="module", params=list(mv.CASES))
def case(request):
    return request.param, mv.build_case(request.param), gc.load_golden(request.param)


def _tensors(c):
    return {k: torch.from_numpy(v) for k, v in c["params"].items()}, torch.from_numpy(c["edge_feat"])


def test_oracle_matches_reference_golden(case):
    name, c, g = case
    p, ef = _tensors(c)
    st = mo.MemoryState(c["node_feat"].shape[0], 172, 2 * 172 + mv.TIME_FEAT_DIM + c["edge_feat"].shape[1])
    for i, b in enumerate(c["batches"]):
        ns, nd = mo.jodie_forward(p, ef, st, b["src"], b["neg"], b["t"], None, False, c["shifts"])
        ps, pd = mo.jodie_forward(p, ef, st, b["src"], b["dst"], b["t"], b["eid"], True, c["shifts"])
        for tag, v in (("neg_src", ns), ("neg_dst", nd), ("pos_src", ps), ("pos_dst", pd)):
            close(v.numpy(), g[f"b{i}_{tag}"], f"{name} batch {i} {tag}")
    close(st.M.numpy(), g["final_memory"], name + " memory")
    close(st.U.numpy(), g["final_last_update"], name + " last update")
    assert np.abs(g["final_memory"]).max() > 0.5 and g["final_last_update"].max() > 0          # the run moved the bank


def test_state_dict_matches_reference_and_loads_strictly(case):
    name, c, g = case
    m = dyglib_amd.JODIE(c["node_feat"], c["edge_feat"], None, time_feat_dim=mv.TIME_FEAT_DIM, **mv.model_kwargs(c))
    assert sorted(m.state_dict().keys()) == g["state_dict_keys"].tolist()
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == syn.jodie_param_shapes(c["node_feat"].shape[0])
    assert {k: v.shape for k, v in c["params"].items()} == {k: s for k, s in syn.jodie_param_shapes(c["node_feat"].shape[0]).items() if "memory_bank" not in k}
    sd = {k: torch.zeros(s) for k, s in syn.jodie_param_shapes(c["node_feat"].shape[0]).items()}          # a reference checkpoint's keys and shapes
    sd.update({k: torch.from_numpy(v) for k, v in c["params"].items()})
    m.load_state_dict(sd, strict=True)
    assert m.memory_bank.node_memories is m.memory_updater.memory_bank.node_memories
    assert (m.src_node_mean_time_shift, m.src_node_std_time_shift, m.dst_node_mean_time_shift_dst, m.dst_node_std_time_shift) == c["shifts"]


def test_constructor_and_refusals():
    c = mv.build_case("jodie_gen")
    nf, ef = c["node_feat"], c["edge_feat"]
    with pytest.raises(ValueError):
        dyglib_amd.JODIE(nf, ef, None, 100, model_name="DyRep")
    with pytest.raises(ValueError):
        dyglib_amd.JODIE(nf, ef, None, 100, model_name="TGN")
    m = dyglib_amd.JODIE(nf, ef, None, 100, model_name="JODIE", device="cpu")
    assert m.model_name == "JODIE" and m.memory_dim == 172 and m.message_dim == 2 * 172 + 100 + ef.shape[1]
    with pytest.raises(AssertionError):
        m.set_neighbor_sampler(None)
    for f in ("__init_memory_bank__", "backup_memory_bank", "reload_memory_bank", "detach_memory_bank"):
        assert callable(getattr(m.memory_bank, f))
    b = c["batches"][0]
    m.eval()
    with torch.no_grad(), pytest.raises(_capi.DygnnError):                                  # no CPU fallback
        m.compute_src_dst_node_temporal_embeddings(b["src"], b["dst"], b["t"], b["eid"], True)
    with pytest.raises(NotImplementedError, match="follow-up"):                             # eval mode, autograd recording on trainable parameters
        m.compute_src_dst_node_temporal_embeddings(b["src"], b["dst"], b["t"], b["eid"], True)
    m.train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="follow-up"):            # training mode
        m.compute_step_embeddings(b["src"], b["dst"], b["src"], b["neg"], b["t"], b["eid"])
    # the names of the existing entry points keep refusing
    with pytest.raises(NotImplementedError):
        dyglib_amd.MemoryModel(nf, ef, None, 100, model_name="JODIE")
    with pytest.raises(ValueError, match="Wrong value for model_name"):
        dyglib_amd.evaluate_memory_model_link_prediction("TGN", torch.nn.Sequential(m, dyglib_amd.MergeLayer(172, 172, 172, 1)), None, [],
                                                         dyglib_amd.NegativeEdgeSampler(c["src"], c["dst"], seed=0), None, torch.nn.BCELoss())


def test_entry_points_are_exported():
    for n in ("JODIE", "compute_src_dst_node_time_shifts", "evaluate_memory_model_link_prediction"):
        assert n in dyglib_amd.__all__ and getattr(dyglib_amd, n).__name__ == n


def test_time_shifts_are_bit_equal_to_the_reference(case):
    name, c, g = case
    n = c["n_train"]
    got = dyglib_amd.compute_src_dst_node_time_shifts(c["src"][:n], c["dst"][:n], c["t"][:n])
    assert all(isinstance(x, np.float64) for x in got)
    assert np.array(got, dtype=np.float64).tobytes() == g["time_shifts"].tobytes()
    assert not np.isclose(got[0], 0.0) and not np.isclose(got[1], 1.0)                         # the fixtures pin constants that are not the defaults


@pytest.mark.parametrize("seed,n,nodes,integer", [(1, 1, 3, False), (2, 500, 7, False), (3, 2000, 300, True), (4, 64, 1, False)])
def test_time_shifts_against_the_loop(seed, n, nodes, integer):
    rs = np.random.RandomState(seed)
    s, d = rs.randint(1, nodes + 1, n), rs.randint(1, nodes + 1, n)
    t = np.sort(rs.randint(0, 50, n).astype(np.float64) if integer else rs.uniform(0, 1e6, n))
    got, want = dyglib_amd.compute_src_dst_node_time_shifts(s, d, t), mv.reference_time_shifts(s, d, t)
    assert np.array(got).tobytes() == np.array(want, dtype=np.float64).tobytes()


def test_recipes_cover_what_the_kernels_branch_on():
    """conditions on the recipes (change a recipe, not an assertion, if one fails)"""
    profiles = {name: mv.pending_profile(mv.build_case(name)["batches"]) for name in mv.CASES}
    for name, prof in profiles.items():
        assert prof[0][0] == 0, name                                                        # batch 0: no pending message at all
        assert any(p > 0 and q > 0 for p, q in prof[1:]), name                              # a later batch with roots of both kinds
    assert any(p % 4 for prof in profiles.values() for p, _ in prof)                        # a pending-row count that is no multiple of the 4-row block
    hub = mv.build_case("jodie_hub")["batches"]
    assert any(len(np.intersect1d(b["src"], b["dst"])) > 0 for b in hub)                    # one node in both roles within a batch
    assert any(np.unique(np.concatenate([b["src"], b["dst"]]), return_counts=True)[1].max() >= 3 for b in hub)
    for name in mv.CASES:
        assert not np.isclose(mv.build_case(name)["shifts"], [0.0, 1.0, 0.0, 1.0]).any()


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
# The refusal tests hand host pointers to the entry points: every case must be refused before a copy or a launch.  Were a check ever misplaced, a
# kernel would receive them, which on a GPU machine could fault a shared card: CPU machines only, as in tests/test_capi_cpu.py.
cpu_only = pytest.mark.skipif(torch.cuda.is_available(), reason="hands host pointers to the library: CPU machines only")


def _call(lib, cfg, batch=4, n_pos=4, ws_bytes=None, null=(), num_nodes=10):
    """dygnn_jodie_forward_step on host dummies: every refusal below happens before anything is launched or dereferenced"""
    Fn, Fe, Ft = (min(x, 32) for x in (cfg.node_feat_dim, cfg.edge_feat_dim, cfg.time_feat_dim))      # (a refused config's buffers are never read)
    Dm = 2 * Fn + Ft + Fe
    f = lambda *s: np.zeros(s, dtype=np.float32)
    a = dict(time_w=f(Ft), time_b=f(Ft), w_ih=f(Fn, Dm), w_hh=f(Fn, Fn), b_ih=f(Fn), b_hh=f(Fn), proj_w=f(Fn), proj_b=f(Fn), edge_feat=f(8, Fe),
             memory=f(num_nodes, Fn), last_update=f(num_nodes), msg=f(num_nodes, Dm), msg_time=np.zeros(num_nodes), has_msg=np.zeros(num_nodes, dtype=np.int32),
             src=np.ones(max(batch, 1), dtype=np.int64), dst=np.ones(max(batch, 1), dtype=np.int64), times=np.zeros(max(batch, 1)),
             eids=np.zeros(max(batch, 1), dtype=np.int64), out=f(2, max(batch, 1), Fn), ws=np.zeros(1 << 16, dtype=np.uint8))
    p = {k: (None if k in null else v.ctypes.data) for k, v in a.items()}
    rnn = _capi.RnnWeights(p["w_ih"], p["w_hh"], p["b_ih"], p["b_hh"])
    st = _capi.TgnState(num_nodes, p["memory"], p["last_update"], p["msg"], p["msg_time"], p["has_msg"])
    out_dst = None if p["out"] is None else p["out"] + 4 * max(batch, 1) * Fn
    rc = lib.dygnn_jodie_forward_step(C.byref(cfg), p["time_w"], p["time_b"], C.byref(rnn), p["proj_w"], p["proj_b"], 0.5, 2.0, 0.25, 3.0, p["edge_feat"],
                                      C.byref(st), p["src"], p["dst"], p["times"], p["eids"], batch, n_pos, p["out"], out_dst, p["ws"],
                                      len(a["ws"]) if ws_bytes is None else ws_bytes, None)
    return rc, lib.dygnn_last_error().decode()


@cpu_only
def test_c_abi_refuses_bad_arguments():
    lib = _capi.load()
    cfg = _capi.TgatConfig(16, 8, 8, 1, 2, 10)
    for n_pos in (-1, 5):
        rc, msg = _call(lib, cfg, batch=4, n_pos=n_pos)
        assert rc == -1 and "n_positive must be in [0, batch]" in msg
    for null, what in ((("w_ih",), "null RNN weights"), (("b_hh",), "null RNN weights"), (("proj_w",), "null weights"), (("time_b",), "null weights"),
                       (("memory",), "bad state"), (("has_msg",), "bad state"), (("edge_feat",), "bad arguments"), (("ws",), "bad arguments"),
                       (("src",), "null pointer"), (("out",), "null pointer"), (("eids",), "edge_ids required")):
        rc, msg = _call(lib, cfg, null=null)
        assert rc == -1 and what in msg, (null, rc, msg)
    rc, msg = _call(lib, cfg, null=("eids",), n_pos=0, ws_bytes=0)          # a negative call needs no edge ids: the next check speaks
    assert rc == -4 and "workspace too small" in msg
    rc, msg = _call(lib, cfg, ws_bytes=lib.dygnn_jodie_workspace_bytes(C.byref(cfg), 10, 4) - 1)
    assert rc == -4 and "workspace too small" in msg
    for bad, val in ((_capi.TgatConfig(18, 8, 8, 1, 2, 10), "node_feat_dim = 18"), (_capi.TgatConfig(16, 6, 8, 1, 2, 10), "edge_feat_dim = 6"),
                     (_capi.TgatConfig(16, 8, 10, 1, 2, 10), "time_feat_dim = 10"), (_capi.TgatConfig(4096, 4096, 4096, 1, 2, 10), "= 16384")):
        assert lib.dygnn_jodie_workspace_bytes(C.byref(bad), 10, 4) == 0
        assert val in lib.dygnn_last_error().decode()
        rc, msg = _call(lib, bad, batch=0, n_pos=0)
        assert rc == -3 and val in msg
    assert _call(lib, cfg, batch=0, n_pos=0)[0] == 0                          # an empty batch: nothing launched


def test_workspace_does_not_depend_on_the_number_of_nodes():
    lib = _capi.load()
    cfg = _capi.TgatConfig(172, 172, 100, 1, 2, 10)
    small, big = lib.dygnn_jodie_workspace_bytes(C.byref(cfg), 10, 400), lib.dygnn_jodie_workspace_bytes(C.byref(cfg), 10 ** 7, 400)
    assert small == big > 0
    assert big < 2 * 1024 * 1024 + 2 * 400 * (172 + 2) * 4 + 4096          # the packed cell (< 1 MiB) + three per-row arrays
    assert lib.dygnn_jodie_workspace_bytes(C.byref(cfg), 10, 800) > big


# ---- DyRep ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(mv.DYREP_CASES))
def dyrep_case(request):
    return request.param, mv.build_dyrep_case(request.param), gc.load_golden(request.param)


def test_dyrep_oracle_matches_reference_golden(dyrep_case):
    from oracle import dygformer_oracle as orc
    name, c, g = dyrep_case
    d, cfg = c["data"], c["cfg"]
    p, ef, nf = {k: torch.from_numpy(v) for k, v in c["params"].items()}, torch.from_numpy(c["edge_feat"]), torch.from_numpy(c["node_feat"])
    adj = orc.OracleAdjacency(d.src_node_ids, d.dst_node_ids, d.edge_ids, d.node_interact_times)
    st = mo.MemoryState(nf.shape[0], 172, 2 * 172 + 100 + ef.shape[1])
    for i, b in enumerate(c["batches"]):
        ns, nd = mo.dyrep_forward(p, nf, ef, adj, st, b["src"], b["neg"], b["t"], None, False, cfg["num_layers"], cfg["num_neighbors"])
        ps, pd = mo.dyrep_forward(p, nf, ef, adj, st, b["src"], b["dst"], b["t"], b["eid"], True, cfg["num_layers"], cfg["num_neighbors"])
        for tag, v in (("neg_src", ns), ("neg_dst", nd), ("pos_src", ps), ("pos_dst", pd)):
            close(v.numpy(), g[f"b{i}_{tag}"], f"{name} batch {i} {tag}")
    close(st.M.numpy(), g["final_memory"], name + " memory")
    close(st.U.numpy(), g["final_last_update"], name + " last update")
    assert np.abs(g["final_memory"]).max() > 0.5
    for tag in mv.DYREP_RANDOM_TAGS:          # the random strategies' runs differ from the `recent` one: the sampled neighbours reach the memories
        assert np.abs(gc.load_golden(f"{name}_{tag}")["final_memory"] - g["final_memory"]).max() > 1e-3


def test_dyrep_state_dict_constructor_and_refusals(dyrep_case):
    from dyglib_amd import NeighborSampler
    from dyglib_amd.temporal_csr import TemporalCSR
    name, c, g = dyrep_case
    d, cfg = c["data"], c["cfg"]
    sampler = NeighborSampler(None, "recent", seed=0, csr=TemporalCSR.from_interactions(d.src_node_ids, d.dst_node_ids, d.edge_ids, d.node_interact_times), device="cpu")
    m = dyglib_amd.DyRep(c["node_feat"], c["edge_feat"], sampler, time_feat_dim=100, model_name="DyRep", num_layers=cfg["num_layers"], num_heads=2, device="cpu")
    shapes = syn.dyrep_param_shapes(c["node_feat"].shape[0], num_layers=cfg["num_layers"])
    assert sorted(m.state_dict().keys()) == g["state_dict_keys"].tolist()
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == shapes
    sd = {k: torch.zeros(s) for k, s in shapes.items()}
    sd.update({k: torch.from_numpy(v) for k, v in c["params"].items()})
    m.load_state_dict(sd, strict=True)
    with pytest.raises(ValueError):
        dyglib_amd.DyRep(c["node_feat"], c["edge_feat"], sampler, 100, model_name="JODIE")
    with pytest.raises(NotImplementedError):
        dyglib_amd.MemoryModel(c["node_feat"], c["edge_feat"], sampler, 100, model_name="DyRep")
    m.set_neighbor_sampler(sampler)
    b = c["batches"][0]
    m.eval()
    with torch.no_grad(), pytest.raises(_capi.DygnnError):
        m.compute_src_dst_node_temporal_embeddings(b["src"], b["dst"], b["t"], b["eid"], True, cfg["num_neighbors"])
    with pytest.raises(NotImplementedError, match="follow-up"):
        m.compute_src_dst_node_temporal_embeddings(b["src"], b["dst"], b["t"], b["eid"], True, cfg["num_neighbors"])
    m.train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="follow-up"):
        m.compute_step_embeddings(b["src"], b["dst"], b["src"], b["neg"], b["t"], b["eid"], cfg["num_neighbors"])
    assert "DyRep" in dyglib_amd.__all__ and dyglib_amd.DyRep.__name__ == "DyRep"


@cpu_only
def test_dyrep_c_abi_refuses_bad_arguments():
    lib = _capi.load()
    cfg = _capi.TgatConfig(16, 8, 8, 1, 2, 10)
    Fn, Dm, N, B = 16, 48, 10, 4
    f = lambda *s: np.zeros(s, dtype=np.float32)
    keep = dict(w_ih=f(Fn, Dm), w_hh=f(Fn, Fn), b=f(Fn), tw=f(8), mem=f(N, Fn), lu=f(N), msg=f(N, Dm), mt=np.zeros(N), has=np.zeros(N, dtype=np.int32),
                ids=np.ones(B, dtype=np.int64), t=np.zeros(B), out=f(2, B, Fn), feat=f(N, Fn), ws=np.zeros(64, dtype=np.uint8))
    P = {k: v.ctypes.data for k, v in keep.items()}
    w = _capi.TgatWeights()
    w.time_w = w.time_b = P["tw"]
    st = _capi.TgnState(N, P["mem"], P["lu"], P["msg"], P["mt"], P["has"])

    def call(rnn, n_pos, eids=P["ids"], ws_bytes=64, fn=lib.dygnn_dyrep_forward_step, graph=None):
        rc = fn(C.byref(cfg), C.byref(w), C.byref(rnn), graph, P["feat"], P["feat"], C.byref(st), P["ids"], P["ids"], P["t"], eids, B, n_pos, P["out"],
                P["out"] + 4 * B * Fn, P["ws"], ws_bytes, None)
        return rc, lib.dygnn_last_error().decode()
    good = _capi.RnnWeights(P["w_ih"], P["w_hh"], P["b"], P["b"])
    for n_pos in (-1, 5):
        rc, msg = call(good, n_pos)
        assert rc == -1 and "n_positive must be in [0, batch]" in msg
    rc, msg = call(_capi.RnnWeights(P["w_ih"], None, P["b"], P["b"]), 0)
    assert rc == -1 and "null RNN weights" in msg
    rc, msg = call(good, 4, eids=None)
    assert rc == -1 and "edge_ids required" in msg
    rc, msg = call(good, 0)
    assert rc == -4 and "workspace too small" in msg
    rc, msg = call(good, 4, fn=lib.dygnn_dyrep_forward_levels)
    assert rc == -1 and "levels is NULL" in msg
    assert lib.dygnn_dyrep_workspace_bytes(C.byref(cfg), N, B) > lib.dygnn_jodie_workspace_bytes(C.byref(cfg), N, B)
    bad = _capi.TgatConfig(18, 8, 8, 1, 2, 10)
    assert lib.dygnn_dyrep_workspace_bytes(C.byref(bad), N, B) == 0
