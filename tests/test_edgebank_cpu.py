"""EdgeBank without a GPU: the CPU oracle against the reference's own outputs (tests/golden/edgebank_*.npz), the boundary (exports, header
against ctypes, host-side argument checks of every entry point with no kernel launched), the error behaviour of the Python layer, and the
rule that fixed_proportion's window start is numpy's own np.quantile on the host."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import dyglib_amd
from dyglib_amd import _build, _capi, edgebank as eb
from tests import edgebank_cases as ec
from tests import edgebank_oracle as eo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
cpu_only = pytest.mark.skipif(torch.cuda.is_available(), reason="hands dummy device pointers to the library / needs a machine without a GPU")
DUMMY = 1 << 20


@pytest.fixture(scope="module")
def lib():
    _build.build(verbose=False)
    return _capi.load()


def _oracle_batches(c, mode, window_mode, neg_dst):
    test, out, o = c["test"], [], 0
    for b, idx in enumerate(c["batches"]):
        src = test.src_node_ids[idx]
        p, n = eo.edge_bank_link_prediction(ec.history_of(c, b), (src, test.dst_node_ids[idx]), (src, neg_dst[o:o + len(idx)]), mode, window_mode,
                                            ec.TEST_RATIO)
        out.append(np.concatenate([p, n]))
        o += len(idx)
    return out


@pytest.mark.parametrize("name", list(ec.CASES))
def test_oracle_matches_reference_fixtures(name):
    c, g = ec.build_case(name), ec.load_golden(name)
    assert len(g["neg_dst"]) == sum(len(i) for i in c["batches"])
    for key, (mode, window_mode) in zip(ec.MODE_KEYS, ec.MODES):
        batches = _oracle_batches(c, mode, window_mode, g["neg_dst"])
        np.testing.assert_array_equal(np.concatenate(batches), g[f"{key}|prob"])                  # exact
        for b, s in enumerate(batches):
            y = np.concatenate([np.ones(len(s) // 2), np.zeros(len(s) // 2)])
            assert abs(eo.bce_loss(s, y) - g[f"{key}|loss"][b]) <= 1e-5
        if f"{key}|start" in g:
            assert (g[f"{key}|gap"] >= ec.MARGIN).all()                                           # the margin condition of the window modes
            for b in range(len(c["batches"])):
                h = ec.history_of(c, b)
                start = eo.window_start(h.src_node_ids, h.dst_node_ids, h.node_interact_times, window_mode, ec.TEST_RATIO)
                span = h.node_interact_times.max() - h.node_interact_times.min()
                assert abs(start - g[f"{key}|start"][b]) <= 1e-9 * span                            # far inside the margin


def test_oracle_matches_hand_cases_and_reference():
    g = ec.load_golden("hand")
    empty = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    for h in ec.hand_cases():
        class Hist:
            src_node_ids, dst_node_ids, node_interact_times = h["history"]
        p, n = eo.edge_bank_link_prediction(Hist, h["queries"], empty, h["mode"], h["window_mode"], h["proportion"])
        assert p.tolist() == h["expected"] == g[f"{h['name']}|prob"].tolist(), h["name"]
        assert len(n) == 0
    assert float(g["tie_at_start|start"][0]) == 2.0 and float(g["repeat_interval|start"][0]) == 7.5


def test_names_are_exported():
    for name in ("edge_bank_link_prediction", "evaluate_edge_bank_link_prediction"):
        assert name in dyglib_amd.__all__
        assert getattr(dyglib_amd, name) is getattr(eb, name)


def test_header_agrees_with_ctypes(lib):
    header = open(os.path.join(ROOT, "include", "dygnn.h")).read()
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double, "dygnn_stream_t": C.c_void_p, "size_t": C.c_size_t,
             "uint64_t": C.c_uint64, "int": C.c_int}
    names = [n for n in _capi.SIGNATURES if n.startswith("dygnn_edgebank_")]
    assert sorted(names) == sorted(["dygnn_edgebank_table_bytes", "dygnn_edgebank_home_slot", "dygnn_edgebank_reset", "dygnn_edgebank_insert",
                                    "dygnn_edgebank_query", "dygnn_edgebank_evaluate"])
    for name in names:
        m = re.search(r"^(\w+) " + name + r"\(([^;]*)\);", header, re.M)
        assert m, name
        res, args = _capi.SIGNATURES[name]
        assert ctype[m.group(1)] is res, name
        want = []
        for a in m.group(2).replace("\n", " ").split(","):
            a = a.strip()
            if "dygnn_edgebank*" in a:
                want.append(C.POINTER(_capi.EdgeBank))
            elif a.startswith("const int64_t* hist_len_host"):
                want.append(_capi.c_i64p)
            elif "*" in a:
                want.append(C.c_void_p)
            else:
                want.append(ctype[a.split()[0]])
        assert want == args, (name, want, args)
        assert hasattr(lib, name)
    fields = re.search(r"typedef struct dygnn_edgebank \{(.*?)\} dygnn_edgebank;", header, re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [f for f, _ in _capi.EdgeBank._fields_]
    assert C.sizeof(_capi.EdgeBank) == 32


def test_table_sizes_and_hash(lib):
    assert lib.dygnn_edgebank_table_bytes(-1) == 0 and lib.dygnn_edgebank_table_bytes((1 << 30) + 1) == 0       # refused sizes
    for n in (0, 1, 4, 5, 8, 9, 1000, 157474):
        cap = eb.table_capacity(n)
        assert cap >= max(2 * n, 8) and cap & (cap - 1) == 0 and (cap == 8 or cap < 4 * n)
        assert lib.dygnn_edgebank_table_bytes(n) == 64 + 2048 + 28 * cap
    assert eb.table_capacity(5) == 16
    rs = np.random.RandomState(0)
    for s, d, n in zip(rs.randint(0, 1 << 31, 200), rs.randint(0, 1 << 31, 200), rs.randint(0, 100000, 200)):
        assert lib.dygnn_edgebank_home_slot(int(s), int(d), int(n)) == eb.home_slot(s, d, eb.table_capacity(n)) == ec._home_slot(int(s), int(d), eb.table_capacity(n))
    assert lib.dygnn_edgebank_home_slot(1 << 31, 0, 5) == lib.dygnn_edgebank_home_slot(0, -1, 5) == (1 << 64) - 1
    assert [eb.home_slot(s, d, 16) for s, d in ec.colliding_pairs()] == [15, 15, 15, 14, 14, 15]


def _expect(lib, rc, code, fragment):
    assert rc == code, (rc, lib.dygnn_last_error())
    assert fragment in lib.dygnn_last_error().decode(), lib.dygnn_last_error()


@cpu_only
def test_entry_points_validate_before_any_hip_call(lib):
    """Every case must be refused before the first memset or launch: the device pointers are dummies."""
    D = DUMMY
    need = lib.dygnn_edgebank_table_bytes(10)
    tb = lambda buffer=D, nbytes=need, max_edges=10, num_edges=0: _capi.EdgeBank(buffer, nbytes, max_edges, num_edges)
    by = C.byref
    # reset
    _expect(lib, lib.dygnn_edgebank_reset(None, None), -1, "edgebank_reset: null table")
    _expect(lib, lib.dygnn_edgebank_reset(by(tb(buffer=None)), None), -1, "null table buffer")
    _expect(lib, lib.dygnn_edgebank_reset(by(tb(nbytes=need - 1)), None), -4, "table buffer too small")
    _expect(lib, lib.dygnn_edgebank_reset(by(tb(max_edges=-1)), None), -1, "max_edges -1")
    # insert
    ins = lambda t, first, last, src=D, dst=D, tm=D: lib.dygnn_edgebank_insert(by(t), src, dst, tm, first, last, None)
    _expect(lib, ins(tb(nbytes=need - 1), 0, 5), -4, "edgebank_insert: table buffer too small")
    _expect(lib, ins(tb(num_edges=3), 0, 5), -1, "first (0) must be the number of edges inserted so far (3)")
    _expect(lib, ins(tb(num_edges=3), 3, 2), -1, "last (2) < first (3)")
    _expect(lib, ins(tb(), 0, 11), -1, "exceeds max_edges (10)")
    _expect(lib, ins(tb(), 0, 5, src=None), -1, "edgebank_insert: null pointer")
    _expect(lib, ins(tb(), 0, 5, tm=None), -1, "edgebank_insert: null pointer")
    _expect(lib, ins(tb(num_edges=11), 11, 12), -1, "num_edges 11 outside")
    t = tb(num_edges=4)
    assert ins(t, 4, 4, src=None, dst=None, tm=None) == 0 and t.num_edges == 4          # an empty range is no work
    # query
    qry = lambda t, mode, wm, H, n=3, qs=D, qd=D, out=D, tm=D: lib.dygnn_edgebank_query(by(t), tm, mode, wm, H, 0.0, qs, qd, n, out, None)
    _expect(lib, qry(tb(nbytes=16), 0, 0, 0), -4, "edgebank_query: table buffer too small")
    _expect(lib, qry(tb(num_edges=4), 0, 0, 5), -1, "H (5) exceeds the 4 edges inserted")
    _expect(lib, qry(tb(num_edges=4), 0, 0, -1), -1, "H (-1)")
    _expect(lib, qry(tb(num_edges=4), 0, 0, 3), -1, "H (3) is not the 4 edges inserted")
    _expect(lib, qry(tb(num_edges=4), 3, 0, 4), -1, "memory mode 3")
    _expect(lib, qry(tb(num_edges=4), -1, 0, 4), -1, "memory mode -1")
    _expect(lib, qry(tb(num_edges=4), 2, 2, 4), -1, "time window mode 2")
    _expect(lib, qry(tb(), 2, 0, 0), -1, "empty sequence")
    _expect(lib, qry(tb(num_edges=4), 0, 0, 4, n=-1), -1, "negative query count")
    _expect(lib, qry(tb(num_edges=4), 0, 0, 4, qs=None), -1, "edgebank_query: null pointer")
    _expect(lib, qry(tb(num_edges=4), 0, 0, 4, out=None), -1, "edgebank_query: null pointer")
    _expect(lib, qry(tb(num_edges=4), 2, 1, 4, tm=None), -1, "repeat_interval needs the history times")
    # evaluate
    def ev(t, hist, mode=0, wm=0, q=6, starts=D, src=D, qs=D, n=None):
        h = np.array(hist, dtype=np.int64)
        return lib.dygnn_edgebank_evaluate(by(t), src, D, D, h.ctypes.data_as(_capi.c_i64p), starts, qs, D, len(h) if n is None else n, q, mode,
                                           wm, D, None)
    _expect(lib, ev(tb(nbytes=need - 1), [4, 6]), -4, "edgebank_evaluate: table buffer too small")
    _expect(lib, ev(tb(), [4, 6], n=-1), -1, "negative size")
    _expect(lib, ev(tb(), [4, 6], q=-1), -1, "negative size")
    _expect(lib, ev(tb(), [4, 6], src=None), -1, "edgebank_evaluate: null pointer")
    _expect(lib, ev(tb(), [4, 6], qs=None), -1, "edgebank_evaluate: null pointer")
    _expect(lib, ev(tb(), [4, 6], mode=5), -1, "memory mode 5")
    _expect(lib, ev(tb(), [4, 6], mode=2, wm=0, starts=None), -1, "fixed_proportion needs the batches' start times")
    _expect(lib, ev(tb(), [6, 4]), -1, "history length of batch 1 (4) is below the 6 edges already inserted")
    _expect(lib, ev(tb(num_edges=5), [4, 6]), -1, "history length of batch 0 (4) is below the 5 edges already inserted")
    _expect(lib, ev(tb(), [4, 11]), -1, "history length of batch 1 (11) exceeds max_edges (10)")
    _expect(lib, ev(tb(), [0, 4], mode=2, wm=1), -1, "empty sequence")
    t = tb(num_edges=2)
    assert ev(t, []) == 0 and t.num_edges == 2                                            # no batches: no work
    # the Python layer maps these to ValueError
    with pytest.raises(ValueError, match="memory mode 3"):
        _capi.check(qry(tb(num_edges=4), 3, 0, 4), ValueError)


class _Hist:
    def __init__(self, src, dst, t):
        self.src_node_ids, self.dst_node_ids, self.node_interact_times = np.asarray(src), np.asarray(dst), np.asarray(t, dtype=np.float64)


HIST = _Hist([1, 1, 3], [2, 2, 4], [0.0, 1.0, 2.0])
POS, NEG = (np.array([1]), np.array([2])), (np.array([1]), np.array([4]))


def test_bad_modes_raise_the_reference_messages():
    with pytest.raises(ValueError, match="Not implemented error for edge_bank_memory_mode bogus!"):
        eb.edge_bank_link_prediction(HIST, POS, NEG, "bogus", "fixed_proportion", 0.15)
    with pytest.raises(ValueError, match="Not implemented error for time_window_mode bogus!"):
        eb.edge_bank_link_prediction(HIST, POS, NEG, "time_window_memory", "bogus", 0.15)
    with pytest.raises(ValueError, match="Not implemented error for edge_bank_memory_mode bogus!"):
        eb.evaluate_edge_bank_link_prediction(None, None, None, None, None, edge_bank_memory_mode="bogus")
    with pytest.raises(ValueError, match="Not implemented error for time_window_mode bogus!"):
        eb.evaluate_edge_bank_link_prediction(None, None, None, None, None, edge_bank_memory_mode="time_window_memory", time_window_mode="bogus")
    # the time-window mode is looked at in time_window_memory only: a bad one passes the mode check of the other two
    assert eb._modes("unlimited_memory", "bogus") == (0, 0) and eb._modes("repeat_threshold_memory", "bogus") == (1, 0)
    assert eb._modes("time_window_memory", "repeat_interval") == (2, 1)
    # the oracle says the same
    with pytest.raises(ValueError, match="edge_bank_memory_mode bogus"):
        eo.edge_bank_link_prediction(HIST, POS, NEG, "bogus", "fixed_proportion", 0.15)
    with pytest.raises(ValueError, match="time_window_mode bogus"):
        eo.edge_bank_link_prediction(HIST, POS, NEG, "time_window_memory", "bogus", 0.15)


def test_host_checks_of_the_python_layer():
    empty = _Hist(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0))
    for wm in ("fixed_proportion", "repeat_interval"):
        with pytest.raises(ValueError, match="empty sequence"):
            eb.edge_bank_link_prediction(empty, POS, NEG, "time_window_memory", wm, 0.15)
        with pytest.raises(ValueError):
            eo.edge_bank_link_prediction(empty, POS, NEG, "time_window_memory", wm, 0.15)
    with pytest.raises(ValueError, match=str(2 ** 31)):
        eb.edge_bank_link_prediction(_Hist([1, 2 ** 31], [2, 3], [0.0, 1.0]), POS, NEG, "unlimited_memory", "fixed_proportion", 0.15)
    with pytest.raises(ValueError, match=str(2 ** 31 + 5)):
        eb.edge_bank_link_prediction(HIST, POS, (np.array([1]), np.array([2 ** 31 + 5])), "unlimited_memory", "fixed_proportion", 0.15)
    with pytest.raises(ValueError, match="-7"):
        eb.edge_bank_link_prediction(HIST, (np.array([-7]), np.array([2])), NEG, "unlimited_memory", "fixed_proportion", 0.15)


@cpu_only
def test_cpu_call_is_refused():
    with pytest.raises(_capi.DygnnError):
        eb.edge_bank_link_prediction(HIST, POS, NEG, "unlimited_memory", "fixed_proportion", 0.15)
    from dyglib_amd import NegativeEdgeSampler, get_idx_data_loader
    c = ec.build_case("gen_sorted")
    sampler = NegativeEdgeSampler(c["full"].src_node_ids, c["full"].dst_node_ids, seed=c["neg_seed"])
    loader = get_idx_data_loader(list(range(c["test"].num_interactions)), batch_size=c["batch"], shuffle=False)
    with pytest.raises(_capi.DygnnError):
        eb.evaluate_edge_bank_link_prediction(c["train"], c["val"], loader, sampler, c["test"])


def test_window_start_is_numpys_quantile_on_the_host(monkeypatch):
    """fixed_proportion: start is np.quantile itself, on the host, once per history: bit-equal to the reference's for every history length of
    the fixtures, and computed by numpy's function, not by a restatement."""
    for name in ec.CASES:
        c, g = ec.build_case(name), ec.load_golden(name)
        for b in range(len(c["batches"])):
            t = ec.history_of(c, b).node_interact_times
            got = eb.window_start_time(t, ec.TEST_RATIO)
            assert got == float(np.quantile(t, 1 - ec.TEST_RATIO)) == float(g["window_fixed|start"][b])          # bit-equal
    calls = []
    real = np.quantile
    monkeypatch.setattr(np, "quantile", lambda a, q, *k, **kw: calls.append((len(a), q)) or real(a, q, *k, **kw))
    assert eb.window_start_time(np.arange(5.0), 0.5) == 2.0 and calls == [(5, 0.5)]
    # the other modes never ask for it (checked up to the point where a machine without a GPU is refused)
    calls.clear()
    for mode, wm in (("unlimited_memory", "fixed_proportion"), ("repeat_threshold_memory", "fixed_proportion"), ("time_window_memory", "repeat_interval")):
        try:
            eb.edge_bank_link_prediction(HIST, POS, NEG, mode, wm, 0.15)
        except _capi.DygnnError:
            pass
    assert calls == []
    try:
        eb.edge_bank_link_prediction(HIST, POS, NEG, "time_window_memory", "fixed_proportion", 0.15)
    except _capi.DygnnError:
        pass
    assert calls == [(3, 0.85)]


def test_decreasing_times_are_refused_before_the_gpu_is_needed():
    from dyglib_amd import NegativeEdgeSampler, get_idx_data_loader
    c = ec.build_case("gen_unsorted")                            # its tail is shuffled in time
    sampler = NegativeEdgeSampler(c["full"].src_node_ids, c["full"].dst_node_ids, seed=c["neg_seed"])
    loader = get_idx_data_loader(list(range(c["test"].num_interactions)), batch_size=37, shuffle=False)
    with pytest.raises(ValueError, match="chronological"):
        eb.evaluate_edge_bank_link_prediction(c["train"], c["val"], loader, sampler, c["test"])
