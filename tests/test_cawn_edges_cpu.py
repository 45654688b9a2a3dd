"""The preconditions of tests/test_cawn_edges_gpu.py, without a GPU: the inputs of tests/cawn_edge_cases.py do what they claim.

The hash of k_cawn_pos (dyglib_amd/csrc/cawn.hip) is restated in tests/cawn_edge_cases.py (`slot_of`, `replay_probing`) and its constant is
named there.  That is on purpose: group A's relabelling is derived from this one function.  If the kernel's hash, table size or probing
changes, test_the_kernel_still_hashes_this_way fails; the relabelling (`crowded_ids`, CROWDED_SLOTS) and the figures asserted below then
have to be derived again for the new function, not deleted.  Group A2 (3000 nodes on their natural ids) keeps probing under any hash."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dyglib_amd import _capi, synthetic as syn
from tests import cawn_cases as cc
from tests import cawn_edge_cases as ce
from tests import golden_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pair_replays(sides, pair_a, pair_b):
    return [ce.replay_probing(ce.pair_tree_ids(sides, a, b)) for a, b in zip(pair_a, pair_b)]


def test_the_kernel_still_hashes_this_way():
    src = open(os.path.join(ROOT, "dyglib_amd", "csrc", "cawn.hip")).read()
    assert re.search(r"constexpr int kSlots = 1024;", src)
    assert "(int)((id * 0x9E3779B97F4A7C15ull) >> 54)" in src and ce.HASH_MULT == 0x9E3779B97F4A7C15 and ce.SLOTS == 1024
    assert "slot = (slot + 1) & (kSlots - 1);" in src                                  # linear probing, wrapping to slot 0
    assert ce.slot_of(0) == 0                                                            # the padding id lives in slot 0
    ids = ce.crowded_ids()
    assert len(ids) == 160 and ids[:5].tolist() == [233, 377, 610, 754, 987]
    assert {ce.slot_of(v) for v in ids} == set(ce.CROWDED_SLOTS)
    # consecutive small ids spread perfectly: what every earlier CAWN test ran on
    assert len({ce.slot_of(v) for v in range(400)}) == 400
    assert 700 - len({ce.slot_of(v) for v in range(700)}) == 24 and 1000 - len({ce.slot_of(v) for v in range(1000)}) == 110


def test_a1_relabelled_batch_probes_wraps_and_runs_over_the_padding_id():
    c = ce.a1()
    nat, rel = c["sides"]
    node_map = c["node_map"]
    assert len(np.unique(node_map)) == 151 and node_map[0] == 0 and node_map.max() < 32768          # injective, the padding id stays
    assert np.array_equal(c["node_feat"][1][node_map], c["node_feat"][0]) and not c["node_feat"][1][0].any()
    assert np.abs(c["node_feat"][1]).sum() == np.abs(c["node_feat"][0]).sum()                        # every other row is zero
    assert 3 <= len(c["pair_a"]) <= 6
    for h in range(2):                                               # the same hops through the map: recent sampling does not look at ids
        assert np.array_equal(node_map[nat[2][h][0]], rel[2][h][0]) and np.array_equal(nat[2][h][1], rel[2][h][1])
        assert np.array_equal(nat[2][h][2], rel[2][h][2])
    reps = pair_replays(rel, c["pair_a"], c["pair_b"])
    for r in reps:
        print(r)
    for p in c["full"]:
        assert 120 <= reps[p]["unique"] <= 150 and not reps[p]["zero"]                               # full trees: no padding
        assert reps[p]["longest"] >= 64 and reps[p]["wraps"] >= 1
    assert sum(reps[p]["steps"] for p in c["full"]) > 7000
    m = reps[c["mixed"]]
    assert m["zero"] and m["unique"] >= 33 and m["wraps"] >= 1 and m["over_zero"] >= 1
    assert reps[c["empty"]]["unique"] == 3 and reps[c["empty"]]["zero"]                              # two targets and the padding id
    for r in pair_replays(nat, c["pair_a"], c["pair_b"]):            # the natural-id run is the run that does not probe
        assert r["steps"] == 0


def test_a2_natural_ids_probe_under_this_hash():
    c = ce.a2()
    assert len(c["src"]) == 4
    for r in pair_replays(c["sides"], c["pair_a"], c["pair_b"]):
        print(r)
        assert r["unique"] >= 200 and r["steps"] >= 10


def test_no_earlier_cawn_graph_ever_probed():
    """the gap: on every graph of tests/cawn_cases.py and of tests/test_cawn_gpu.py's against_restatement ALL node ids have distinct home slots,
    so no tree drawn from them takes a probe step"""
    graphs = [gc.build_case(r["graph"])["data"] for r in cc.CASES.values()]
    graphs.append(syn.make_bipartite_graph(60, 9, 6000, seed=3, duplicate_time_every=5)[0])
    for data in graphs:
        n = data.max_node_id + 1
        assert n <= 207 and len({ce.slot_of(v) for v in range(n)}) == n
    for name in cc.CASES:                                            # and the batches themselves, replayed
        c = cc.build_cawn_case(name)
        cfg = c["cawn_cfg"]
        if cfg["strategy"] != "recent":
            continue
        for dst in (c["dst"], c["neg_dst"]):
            sides, pa, pb = ce.batch_sides(c["data"], cfg["W"], cfg["k"], c["src"], dst, c["times"])
            assert all(r["steps"] == 0 for r in pair_replays(sides, pa, pb))


def test_restatement_is_invariant_under_the_relabelling():
    c = ce.a1()
    heads = ce.A_MODEL["heads"]
    out = [ce.restate(c["params"], c["node_feat"][i], c["edge_feat"], c["sides"][i], c["pair_a"], c["pair_b"], heads, taps=True) for i in range(2)]
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][2]["counts"], out[1][2]["counts"])
    assert np.array_equal(c["node_map"][out[0][2]["walk_ids"]], out[1][2]["walk_ids"])
    assert np.abs(out[0][0] - out[0][1]).max() > 0.02 and out[0][2]["counts"][c["full"]].max() > 0.0
    both = (out[0][2]["counts"][..., 0, :].sum(-1) > 0) & (out[0][2]["counts"][..., 1, :].sum(-1) > 0)
    assert both[c["full"]].any() and both[c["mixed"]].any()          # nodes of both trees


@pytest.mark.parametrize("name", list(ce.SHAPES))
def test_shape_configs_are_accepted_and_sit_on_the_edges_they_claim(name):
    c = ce.shape_case(name)
    r = c["cfg"]
    cfg = _capi.CawnConfig(r["Fn"], r["Fe"], r["Ft"], r["P"], r["W"], r["k"], r["heads"], c["node_feat"].shape[0], c["edge_feat"].shape[0])
    lib = _capi.load()
    assert lib.dygnn_cawn_check(C.byref(cfg)) == 0, lib.dygnn_last_error()
    assert 3 <= len(c["src"]) <= 5 and c["node_feat"].shape[1] == r["Fn"] and c["edge_feat"].shape[1] == r["Fe"]
    want = dict(all128_h8=dict(D=512, A=256), all256_h8=dict(D=1024, A=512), P76_h5=dict(A=260), P196_h8=dict(A=320), P204_h6=dict(A=324),
                Ft84_h5=dict(A=300), narrow_h1=dict(D=72, A=36), all16_h2=dict(D=64, A=32), w2_k8=dict(M=64, T=73), w1_k64=dict(M=64, T=65),
                w1_k65=dict(M=65, T=66), w2_k11_full=dict(M=121, T=133))[name]
    assert {k: r[k] for k in want} == want
    head = dict(all256_h8=64, P76_h5=52, Ft84_h5=60, narrow_h1=36)
    assert name not in head or r["A"] // r["heads"] == head[name]
    ids = c["sides"][2][-1][0]
    if r["deep"] or r["graph"] == "a2":                              # no padded key: every queried node has more than k earlier interactions
        assert c["hist_src"].min() > r["k"] and c["hist_dst"].min() > r["k"] and (c["sides"][2][0][0] != 0).all()
        if r["graph"] == "a2":
            assert (ids != 0).mean() > 0.95                          # 266 tree positions, nearly all of them nodes
    else:                                                            # an empty pair beside full walks
        assert c["hist_src"][0] == 0 and c["hist_dst"][0] == 0 and not ids[[0, len(c["src"])]].any() and (ids[1:len(c["src"])] != 0).any()


def test_hand_built_sides_hold_what_the_contract_cases_need():
    c = ce.c_case()
    roots, times, hops = c["sides"]
    assert len(roots) == 6 and hops[0][0].shape == (6, 3) and hops[1][0].shape == (6, 9) and len(set(times[:3]) | set(times[3:])) > 1
    pa, pb = ce.C_PAIRS
    assert (pa[0], pb[0]) == (0, 0) and len({pb[i] for i in range(len(pa)) if pa[i] == 1}) == 3
    assert (pa[4], pb[4]) == (pb[5], pa[5]) and pa[4] != pb[4] and 3 <= len(pa) <= 6
    assert (hops[0][0][0] == 0).any() and (hops[1][0][0] == 0).any()                     # a partial tree
    N, Ne = ce.C_NODE_ROWS, ce.C_EDGE_ROWS
    on, oe = np.concatenate([h[0].ravel() for h in c["oob_sides"][2]]), np.concatenate([h[1].ravel() for h in c["oob_sides"][2]])
    assert roots.max() < N and (on == N).any() and (on == ce.C_FAR_NODE).any() and on.min() >= 0 and ((on > 0) & (on < N)).any()
    assert (oe == Ne).any() and (oe > Ne).any() and (oe < 0).sum() >= 3 and ((oe > 0) & (oe < Ne)).sum() >= 10
    rn, re_ = (np.concatenate([h[i].ravel() for h in c["oob_sides_restated"][2]]) for i in (0, 1))
    assert np.array_equal(rn, on) and np.array_equal(re_, np.where(oe < 0, 0, oe))
    assert c["node_feat"][0].any() and c["edge_feat"][0].any()                           # reading row 0 is not reading zeros
    nfx, efx = c["node_feat_ext"], c["edge_feat_ext"]
    assert nfx.shape[0] == ce.C_FAR_NODE + 1 and np.array_equal(nfx[N:], np.repeat(nfx[:1], nfx.shape[0] - N, 0)) and np.array_equal(nfx[:N], c["node_feat"][:N])
    assert efx.shape[0] == ce.C_FAR_EDGE + 1 and np.array_equal(efx[Ne:], np.repeat(efx[:1], efx.shape[0] - Ne, 0)) and np.array_equal(efx[:Ne], c["edge_feat"][:Ne])
    a, b = ce.OOB_PAIRS
    far = [(ce.pair_tree_ids(c["oob_sides"], x, y) == ce.C_FAR_NODE) for x, y in zip(a, b)]
    T = 13
    assert any(f[:T].any() and f[T:].any() for f in far)             # an out-of-range id in both trees of one pair


def test_restatement_on_the_hand_built_sides():
    c = ce.c_case()
    heads = ce.C_MODEL["heads"]
    pa, pb = ce.C_PAIRS
    a, b, taps = ce.restate(c["params"], c["node_feat"], c["edge_feat"], c["sides"], pa, pb, heads, taps=True)
    assert np.abs(a[1] - a[2]).max() > 1e-3 and np.abs(a[1] - a[3]).max() > 1e-3         # a side's rows depend on its partner: 10 x the bar
    assert np.abs(a[4] - b[5]).max() <= 1e-5 and np.abs(b[4] - a[5]).max() <= 1e-5       # (a, b) and (b, a): the same up to the order of a sum
    both = (taps["counts"][..., 0, :].sum(-1) > 0) & (taps["counts"][..., 1, :].sum(-1) > 0)
    assert both[1:].any(axis=(1, 2, 3)).all()                                            # the ids put in by hand: nodes of both trees
    pa, pb = ce.OOB_PAIRS
    oa, ob = ce.restate(c["params"], c["node_feat_ext"], c["edge_feat_ext"], c["oob_sides_restated"], pa, pb, heads)
    ia, ib = ce.restate(c["params"], c["node_feat"], c["edge_feat"], c["sides"], pa, pb, heads)
    assert np.isfinite(oa).all() and np.abs(oa - ia).max() > 1e-3 and np.abs(ob - ib).max() > 1e-3      # the ids outside matter
