"""dygnn_cawn_forward (dyglib_amd/csrc/cawn.hip) on an MI355X where its earlier tests never went, against tests/cawn_oracle.py on the inputs of
tests/cawn_edge_cases.py (tests/test_cawn_edges_cpu.py proves that those inputs do what they claim):

  A  node ids that collide in k_cawn_pos's hash table: probe chains of more than 100 slots, wraps past slot 1023, chains over the padding id;
  B  feature dims and walk counts on both sides of every tile, chunk and template switch of the kernels;
  C  the C contract on hand-built sides: a side paired with itself, one side with several partners, (a, b) beside (b, a), ids outside the tables.

Every comparison takes the taps of ALL pairs of its batch (3 to 6).  Tolerances are the project's standing ones: tests.parity.close (absolute
1e-4) on embeddings and float taps, walk ids exact, counts 1e-5 (tests/test_cawn_cpu.py derives that bound)."""
import functools

import numpy as np
import pytest

from tests import cawn_edge_cases as ce
from tests import parity
from tests.test_cawn_cpu import COUNT_TOL, check_taps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make_model(data, node_feat, edge_feat, params, Ft, P, W, heads):
    import torch
    from dyglib_amd import CAWN, get_neighbor_sampler
    sampler = get_neighbor_sampler(data, "recent", seed=1, device=DEV)
    m = CAWN(node_feat, edge_feat, sampler, Ft, P, walk_length=W, num_walk_heads=heads, device=DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return m.to(DEV).eval()


def class_call(m, c, k, src=None, dst=None):
    """the drop-in class on a batch, with the taps of all its pairs -> (src_emb, dst_emb, taps) as numpy"""
    import torch
    src, dst = c["src"] if src is None else src, c["dst"] if dst is None else dst
    with torch.no_grad():
        s, d, taps = m.compute_src_dst_node_temporal_embeddings(src, dst, c["times"], num_neighbors=k, taps=len(src))
    return s, d, {key: v.cpu().numpy() for key, v in taps.items()}


def sides_call(m, sides, pair_a, pair_b, k, taps=None):
    """dygnn_cawn_forward on explicit sides and pair lists, through the class's one library call (no id validation on this path)"""
    import torch
    roots, times, hops = sides
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    on_dev = (dev(roots), dev(times), [tuple(dev(x) for x in h) for h in hops])
    with torch.no_grad():
        out = m._forward(on_dev, np.asarray(pair_a, dtype=np.int32), np.asarray(pair_b, dtype=np.int32), k, taps)
    torch.cuda.synchronize()
    return out


def against(name, label, got, want):
    """embeddings and all taps of a batch against the restatement's"""
    parity.close(got[0].cpu().numpy(), want[0], f"{name} side a", label)
    parity.close(got[1].cpu().numpy(), want[1], f"{name} side b", label)
    taps = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in got[2].items()}
    check_taps(name, taps, ce.as_golden(want[2]), label)


# ---- A: colliding node ids --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def a1_runs():
    """the GPU on A1's batch on the natural ids [0] and on the relabelled ids [1]"""
    c = ce.a1()
    A = ce.A_MODEL
    out = []
    for i in range(2):
        m = make_model(c["data"][i], c["node_feat"][i], c["edge_feat"], c["params"], A["Ft"], A["P"], A["W"], A["heads"])
        out.append(class_call(m, c, A["k"], c["src"][i], c["dst"][i]))
    return c, out


def test_a1_colliding_ids_match_the_restatement():
    c, runs = a1_runs()
    want = ce.restate(c["params"], c["node_feat"][1], c["edge_feat"], c["sides"][1], c["pair_a"], c["pair_b"], ce.A_MODEL["heads"], taps=True)
    against("A1 relabelled", "cawn A: colliding ids vs restatement", runs[1], want)


def test_a1_counts_and_walks_equal_the_natural_id_run():
    c, (nat, rel) = a1_runs()
    assert np.array_equal(c["node_map"][nat[2]["walk_ids"]], rel[2]["walk_ids"])
    err = float(np.abs(rel[2]["counts"].astype(np.float64) - nat[2]["counts"]).max())
    print(f"A1 counts, relabelled vs natural ids: max abs err {err:.3e}")
    assert np.array_equal(rel[2]["counts"], nat[2]["counts"])        # integers over k^hop on both runs
    assert nat[2]["counts"].max() > 0.0


def test_a1_embeddings_are_bit_equal_to_the_natural_id_run():
    """The natural-id run takes no probe step.  Counts are integers, the kernel orders the unique ids by their first tree position and not by
    their slot, and every later kernel indexes by position: the relabelling may not change one bit."""
    import torch
    c, (nat, rel) = a1_runs()
    for key in ("feature_out", "position_out", "attn_in", "attn_out"):
        print(f"A1 {key}, relabelled vs natural ids: max abs diff {float(np.abs(rel[2][key] - nat[2][key]).max()):.3e}")
    print(f"A1 embeddings, relabelled vs natural ids: max abs diff {float((rel[0] - nat[0]).abs().max()):.3e} / {float((rel[1] - nat[1]).abs().max()):.3e}")
    assert torch.equal(rel[0], nat[0]) and torch.equal(rel[1], nat[1])


def test_a2_many_nodes_on_natural_ids():
    c = ce.a2()
    A = ce.A_MODEL
    m = make_model(c["data"], c["node_feat"], c["edge_feat"], c["params"], A["Ft"], A["P"], A["W"], A["heads"])
    want = ce.restate(c["params"], c["node_feat"], c["edge_feat"], c["sides"], c["pair_a"], c["pair_b"], A["heads"], taps=True)
    against("A2 3000 nodes", "cawn A: colliding ids vs restatement", class_call(m, c, A["k"]), want)


# ---- B: shapes at the tile and chunk edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ce.SHAPES))
def test_shape_at_a_tile_or_chunk_edge(name):
    """the sibling of tests/test_cawn_gpu.py's against_restatement with edge_feat_dim, time_feat_dim and the taps"""
    c = ce.shape_case(name)
    r = c["cfg"]
    m = make_model(c["data"], c["node_feat"], c["edge_feat"], c["params"], r["Ft"], r["P"], r["W"], r["heads"])
    assert m.walk_encoder.attention_dim == r["A"]
    want = ce.restate(c["params"], c["node_feat"], c["edge_feat"], c["sides"], c["pair_a"], c["pair_b"], r["heads"], taps=True)
    against(f"B {name}", "cawn B: tile and chunk edges vs restatement", class_call(m, c, r["k"]), want)


# ---- C: the C contract on hand-built sides ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def c_model(truncated: bool):
    c = ce.c_case()
    C = ce.C_MODEL
    data = c["data"]                                                 # only for the class's sampler slot: these calls bring their own sides
    nf, ef = (c["node_feat"][:ce.C_NODE_ROWS], c["edge_feat"][:ce.C_EDGE_ROWS]) if truncated else (c["node_feat"], c["edge_feat"])
    return make_model(data, nf, ef, c["params"], C["Ft"], C["P"], C["W"], C["heads"])


def test_pair_lists_self_pair_shared_side_and_both_orders():
    """(s, s); one side named by three pairs with different partners; (a, b) with (b, a): each against the restatement of ITS pair (the two
    count rows of (a, b) and (b, a) are summed in the other order, so they are not compared with each other)"""
    import torch
    c = ce.c_case()
    pa, pb = ce.C_PAIRS
    m, k, heads = c_model(False), ce.C_MODEL["k"], ce.C_MODEL["heads"]
    got = sides_call(m, c["sides"], pa, pb, k, taps=len(pa))
    want = ce.restate(c["params"], c["node_feat"], c["edge_feat"], c["sides"], pa, pb, heads, taps=True)
    against("C pair lists", "cawn C: hand-built sides vs restatement", got, want)
    assert np.abs(want[0][1] - want[0][2]).max() > 1e-3 and np.abs(want[0][1] - want[0][3]).max() > 1e-3      # side 1, once per pair: the partner matters
    counts = got[2]["counts"].cpu().numpy()
    assert np.array_equal(counts[0, 0], counts[0, 1]) and np.array_equal(counts[0, ..., 0, :], counts[0, ..., 1, :])      # (s, s): both trees are one tree
    # independence: the first two pairs alone give the same bits
    two = sides_call(m, c["sides"], pa[:2], pb[:2], k)
    assert torch.equal(two[0], got[0][:2]) and torch.equal(two[1], got[1][:2])


def test_ids_outside_the_tables_read_row_0_and_still_count_as_nodes():
    """include/dygnn.h: ids outside the tables read row 0.  The library gets tables of C_NODE_ROWS / C_EDGE_ROWS rows, node ids at and above
    the one, edge ids at and above the other and negative ones; the restatement gets tables extended with copies of row 0 and edge id 0 for
    a negative one.  An out-of-range node is still its own node in the landing counts."""
    c = ce.c_case()
    pa, pb = ce.OOB_PAIRS
    m, k, heads = c_model(True), ce.C_MODEL["k"], ce.C_MODEL["heads"]
    assert m.node_raw_features.shape[0] == ce.C_NODE_ROWS and m.edge_raw_features.shape[0] == ce.C_EDGE_ROWS
    got = sides_call(m, c["oob_sides"], pa, pb, k, taps=len(pa))
    want = ce.restate(c["params"], c["node_feat_ext"], c["edge_feat_ext"], c["oob_sides_restated"], pa, pb, heads, taps=True)
    against("C out-of-range ids", "cawn C: hand-built sides vs restatement", got, want)
    ids, counts = got[2]["walk_ids"].cpu().numpy(), got[2]["counts"].cpu().numpy()
    far = ids == ce.C_FAR_NODE                                       # [pairs, 2, M, W + 1]
    assert far[1, 0].any() and far[1, 1].any()                       # pair (1, 2): the far id sits in both trees,
    rows = counts[1][far[1]]                                         # [., 2, W + 1]: so both its count rows are non-zero
    assert (rows[:, 0].sum(-1) > 0).all() and (rows[:, 1].sum(-1) > 0).all()
    edge = ids == ce.C_NODE_ROWS                                     # the first id outside the table
    assert edge.any() and (counts[edge].sum((-1, -2)) > 0).all()
    err = float(np.abs(counts.astype(np.float64) - want[2]["counts"]).max())
    assert err <= COUNT_TOL
