"""Seeded recipes and helpers for the CAWN edge tests (tests/test_cawn_edges_cpu.py states their preconditions without a GPU,
tests/test_cawn_edges_gpu.py runs them).  Three groups:

  A  node ids that collide in k_cawn_pos's 1024-slot LDS hash table (dyglib_amd/csrc/cawn.hip): a graph relabelled onto ids whose home slot
     is one of 1021, 1022, 1023, 0, 1 (long probe chains, wraps past slot 1023, chains over slot 0 where the padding id 0 lives), and a
     3000-node graph on its natural ids (a few probe steps per pair whatever the hash function is);
  B  feature dims and walk counts at the edges of the kernels' tiles and chunks (SHAPES);
  C  the C contract of include/dygnn.h on hand-built sides: explicit pair lists, ids outside the tables.

Everything is a SIDE list (roots [n], times [n] float64, per hop (ids, edge ids [n, k^h] int64, times [n, k^h] float32)) plus pair index arrays,
the form dygnn_cawn_forward takes.  `restate` is tests/cawn_oracle.py applied to the sides a pair list gathers; its `counts` is a plain
equality count and knows nothing of hashing.  The hops come from cawn_oracle.OracleSampler ("recent"), so the expected values need no GPU.

`slot_of` / `replay_probing` restate the kernel's hash on the host and NAME ITS CONSTANT: if the hash of k_cawn_pos changes,
tests/test_cawn_edges_cpu.py fails and the relabelling of group A has to be derived again for the new function."""
from __future__ import annotations

import functools

import numpy as np
import torch

from dyglib_amd import synthetic as syn
from tests import cawn_cases as cc
from tests import cawn_oracle as cwo

HASH_MULT = 0x9E3779B97F4A7C15          # k_cawn_pos: slot = (id * HASH_MULT) >> 54, linear probing over kSlots = 1024
SLOTS = 1024
CROWDED_SLOTS = (1021, 1022, 1023, 0, 1)
PARAM_SEED = 5
DEFAULTS = dict(Fn=172, Fe=172, Ft=100, P=172, heads=8)


# ---- the hash table of k_cawn_pos on the host -------------------------------------------------------------------------------------------------
def slot_of(node_id: int) -> int:
    return ((int(node_id) * HASH_MULT) & (2 ** 64 - 1)) >> 54


def replay_probing(ids) -> dict:
    """The kernel's insertions for the 2 T tree ids of a pair, one after the other in tree order (on the GPU they interleave: the figures
    of another order differ a little, the table's content as a set does not).  steps: probe steps of all positions, a repeated id walks its
    chain again; longest: the longest single chain; wraps: steps from slot 1023 to slot 0; over_zero: steps of a non-zero id over the slot
    that holds the padding id 0."""
    table = {}
    out = dict(steps=0, longest=0, wraps=0, over_zero=0)
    for v in ids:
        v = max(int(v), 0)                                            # tree_id clamps a negative id to the padding node
        s, n = slot_of(v), 0
        while s in table and table[s] != v:
            out["wraps"] += s == SLOTS - 1
            out["over_zero"] += table[s] == 0
            s, n = (s + 1) & (SLOTS - 1), n + 1
        table[s] = v
        out["steps"] += n
        out["longest"] = max(out["longest"], n)
    vals = set(table.values())
    out["unique"], out["zero"] = len(vals), 0 in vals
    return out


def crowded_ids(limit: int = 32768) -> np.ndarray:
    """the ids in [1, limit) whose home slot is one of CROWDED_SLOTS, ascending: 233, 377, 610, 754, 987, ..."""
    return np.array([v for v in range(1, limit) if slot_of(v) in CROWDED_SLOTS], dtype=np.int64)


# ---- sides ------------------------------------------------------------------------------------------------------------------------------------
def sample_sides(data, W: int, k: int, nodes, times):
    """the sides (nodes[i], times[i]) with the `recent` hops of the host sampler"""
    nodes, times = np.asarray(nodes, dtype=np.int64), np.asarray(times, dtype=np.float64)
    n, e, t = cwo.OracleSampler(data, "recent", 1).multi_hop(W, nodes, times, k)
    return nodes, times, [(np.asarray(a, np.int64), np.asarray(b, np.int64), np.asarray(c, np.float32)) for a, b, c in zip(n, e, t)]


def batch_sides(data, W, k, src, dst, times):
    """sides [src ; dst] and the pairs (i, B + i): what the drop-in class hands to the library for this batch"""
    B = len(src)
    sides = sample_sides(data, W, k, np.concatenate([src, dst]), np.concatenate([times, times]))
    return sides, np.arange(B, dtype=np.int32), np.arange(B, dtype=np.int32) + B


def pair_tree_ids(sides, a: int, b: int) -> np.ndarray:
    """the 2 T node ids k_cawn_pos hashes for the pair (a, b), in tree order"""
    roots, _, hops = sides
    return np.concatenate([np.concatenate([[roots[s]]] + [h[0][s] for h in hops]) for s in (a, b)])


def restate(params, node_feat, edge_feat, sides, pair_a, pair_b, heads: int, taps: bool = False):
    """tests/cawn_oracle.py pair by pair on the sides the index arrays gather -> numpy (out_a, out_b[, taps of every pair])"""
    P = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for k, v in params.items()}
    nf = torch.from_numpy(np.ascontiguousarray(node_feat, dtype=np.float32))
    ef = torch.from_numpy(np.ascontiguousarray(edge_feat, dtype=np.float32))
    roots, times, hops = sides

    def gather(idx):
        idx = np.asarray(idx, dtype=np.int64)
        return (torch.from_numpy(roots[idx]), torch.from_numpy(times[idx]),
                [(torch.from_numpy(n[idx]), torch.from_numpy(e[idx]), torch.from_numpy(t[idx])) for n, e, t in hops])

    ra, ta, ha = gather(pair_a)
    rb, tb, hb = gather(pair_b)
    la, lb = cwo.tree_levels(ra, ha), cwo.tree_levels(rb, hb)
    tp = {k: [] for k in cwo.TAP_KEYS} if taps else None
    with torch.no_grad():
        a = cwo.encode_side(P, nf, ef, ra, ta, ha, la, lb, heads, tp)
        b = cwo.encode_side(P, nf, ef, rb, tb, hb, la, lb, heads, tp)
    if not taps:
        return a.numpy(), b.numpy()
    return a.numpy(), b.numpy(), {k: torch.stack(v, dim=1).numpy() for k, v in tp.items()}


def as_golden(taps: dict) -> dict:
    """the restatement's taps under the names tests.test_cawn_cpu.check_taps reads"""
    return {"tap_" + k: v for k, v in taps.items()}


# ---- A: colliding node ids --------------------------------------------------------------------------------------------------------------------
A_MODEL = dict(W=2, k=11, P=24, heads=4, Ft=cc.TIME_FEAT_DIM)


def relabel(data, node_feat, node_map):
    """the same graph on the node ids node_map[v]: InteractionData and the node feature rows scattered to the new ids (row 0 stays zero)"""
    nf = np.zeros((int(node_map.max()) + 1, node_feat.shape[1]), dtype=np.float32)
    nf[node_map[1:]] = node_feat[1:]
    return syn.InteractionData(node_map[data.src_node_ids], node_map[data.dst_node_ids], data.node_interact_times, data.edge_ids, data.labels), nf


@functools.lru_cache(maxsize=None)
def a1():
    """dict(data, node_feat: [natural, relabelled], edge_feat, node_map, src, dst, times, full, mixed, empty, params, sides: [natural,
    relabelled], pair_a, pair_b): three late pairs queried past the end of the stream (`full`: 122 to 127 unique ids each on full trees), one
    mid-stream pair (`mixed`) whose trees hold padding zeros and at least 32 unique ids and whose chains wrap and run over the padding id,
    one pair with empty histories (`empty`)."""
    data, nf, ef = syn.make_general_graph(150, 3000, seed=22)
    targets = crowded_ids()
    assert len(targets) >= 150
    node_map = np.concatenate([[0], targets[:150]]).astype(np.int64)
    data2, nf2 = relabel(data, nf, node_map)
    W, k = A_MODEL["W"], A_MODEL["k"]
    E, t = data.num_interactions, data.node_interact_times
    # the mid-stream pair: the first interaction of the candidates that does what the recipe claims on the relabelled ids
    cand = np.arange(100, 500)
    sides, pa, pb = batch_sides(data2, W, k, data2.src_node_ids[cand], data2.dst_node_ids[cand], t[cand])
    mid = None
    for i in range(len(cand)):
        ids = pair_tree_ids(sides, pa[i], pb[i])
        if (ids == 0).any() and len(np.unique(ids[ids != 0])) >= 32:
            r = replay_probing(ids)
            if r["wraps"] >= 1 and r["over_zero"] >= 1:
                mid = int(cand[i])
                break
    assert mid is not None
    idx = np.array([E - 1, E - 2, E - 3, mid, 0])
    times = t[idx].copy()
    times[:3] = t.max() + 1.0
    times[4] = t.min() - 1.0
    out = dict(data=[data, data2], node_feat=[nf, nf2], edge_feat=ef, node_map=node_map, times=times, full=[0, 1, 2], mixed=3, empty=4,
               params=syn.make_cawn_params(PARAM_SEED, A_MODEL["P"], W, A_MODEL["heads"]), src=[], dst=[], sides=[])
    for d in (data, data2):
        src, dst = d.src_node_ids[idx].astype(np.int64), d.dst_node_ids[idx].astype(np.int64)
        sides, pa, pb = batch_sides(d, W, k, src, dst, times)
        out["src"].append(src), out["dst"].append(dst), out["sides"].append(sides)
    out["pair_a"], out["pair_b"] = pa, pb
    return out


@functools.lru_cache(maxsize=None)
def a2():
    """3000 nodes on their natural ids, the last four interactions queried past the end: 232 to 247 unique ids a pair"""
    data, nf, ef = syn.make_general_graph(3000, 40000, seed=21)
    E = data.num_interactions
    idx = np.arange(E - 4, E)
    src, dst = data.src_node_ids[idx].astype(np.int64), data.dst_node_ids[idx].astype(np.int64)
    times = np.full(4, data.node_interact_times.max() + 1.0)
    sides, pa, pb = batch_sides(data, A_MODEL["W"], A_MODEL["k"], src, dst, times)
    return dict(data=data, node_feat=nf, edge_feat=ef, src=src, dst=dst, times=times, sides=sides, pair_a=pa, pair_b=pb,
                params=syn.make_cawn_params(PARAM_SEED, A_MODEL["P"], A_MODEL["W"], A_MODEL["heads"]))


# ---- B: shapes at the tile and chunk edges ----------------------------------------------------------------------------------------------------
# name -> what differs from DEFAULTS, W = 2, k = 4 (16 walks; five pairs are 160 walk rows: three 64-row tiles, the last one half full).
# `deep`: every queried node has more than k earlier interactions, so no key of the attention is padding.  `graph`: "a2" is A2's graph.
SHAPES = {
    # every segment [node | time | edge | position] exactly one 128-column chunk; A = 256 fills <4,4>; H = 256: four full unit tiles
    "all128_h8": dict(Fn=128, Fe=128, Ft=128, P=128),
    # two full chunks per segment; A = 512 and head size 64, both the maximum; 8 unit tiles; the largest k_cawn_pos LDS
    "all256_h8": dict(Fn=256, Fe=256, Ft=256, P=256),
    "P76_h5": dict(P=76, heads=5),            # A = 260: the first width of <5,2>, its last column tile holds 4 columns; head size 52
    "P196_h8": dict(P=196),                   # A = 320: <5,2> full
    "P204_h6": dict(P=204, heads=6),          # A = 324: the first width of <8,2>
    "Ft84_h5": dict(Ft=84, heads=5),          # A = 300, head size 60; the time segment is no multiple of 16
    "narrow_h1": dict(Fn=32, Fe=16, Ft=16, P=8, heads=1),      # D = 72 in one chunk; one head of 36; Hp = 4; 32 output columns
    "all16_h2": dict(Fn=16, Fe=16, Ft=16, P=16, heads=2),      # D = 64, A = 32
    "w2_k8": dict(W=2, k=8),                  # M = 64: one key per lane on the M > 64 false side; a sequence is exactly one 64-row tile
    "w1_k64": dict(W=1, k=64, deep=True),     # the two sides of the two-keys-per-lane switch;
    "w1_k65": dict(W=1, k=65, deep=True),     # at 65 only lane 0 holds a second key
    "w2_k11_full": dict(W=2, k=11, graph="a2"),      # M = 121, T = 133: 266 tree positions, a second trip of the tree scan, on full trees
}


def shape_config(name: str) -> dict:
    r = dict(DEFAULTS, W=2, k=4, deep=False, graph="bip")
    r.update(SHAPES[name])
    r["D"] = r["Fn"] + r["Fe"] + r["Ft"] + r["P"]
    r["A"] = syn.cawn_attention_dim(r["D"], r["heads"])
    r["M"] = r["k"] ** r["W"]
    r["T"] = 1 + r["k"] + (r["k"] ** 2 if r["W"] == 2 else 0)
    return r


@functools.lru_cache(maxsize=None)
def shape_case(name: str) -> dict:
    """dict(cfg, data, node_feat, edge_feat, src, dst, times, hist_src, hist_dst, params, sides, pair_a, pair_b)"""
    r = shape_config(name)
    rs = np.random.RandomState(4)
    if r["graph"] == "a2":
        c = a2()
        data, src, dst, times = c["data"], c["src"], c["dst"], c["times"]
        nf, ef = c["node_feat"], c["edge_feat"]
    else:
        data, nf, ef = syn.make_bipartite_graph(60, 9, 6000, seed=3, duplicate_time_every=5, edge_feat_dim=r["Fe"])
        nf = (0.5 * rs.standard_normal((nf.shape[0], r["Fn"]))).astype(np.float32)
        nf[0] = 0.0
        t = data.node_interact_times
        if r["deep"]:                                                 # the last three interactions whose two nodes have long histories
            late = np.arange(data.num_interactions - 300, data.num_interactions)
            hs, hd = (cc.history_lengths(data, x[late], t[late]) for x in (data.src_node_ids, data.dst_node_ids))
            idx = late[(hs > r["k"]) & (hd > r["k"])][-3:]
            times = t[idx].astype(np.float64)
        else:
            idx = rs.randint(0, data.num_interactions, 5)
            times = t[idx].astype(np.float64)
            times[0] = t.min() - 1.0                                  # both histories empty
        src, dst = data.src_node_ids[idx].astype(np.int64), data.dst_node_ids[idx].astype(np.int64)
    sides, pa, pb = batch_sides(data, r["W"], r["k"], src, dst, times)
    return dict(cfg=r, data=data, node_feat=nf, edge_feat=ef, src=src, dst=dst, times=times, hist_src=cc.history_lengths(data, src, times),
                hist_dst=cc.history_lengths(data, dst, times), sides=sides, pair_a=pa, pair_b=pb,
                params=syn.make_cawn_params(PARAM_SEED, r["P"], r["W"], r["heads"], node_feat_dim=r["Fn"], edge_feat_dim=r["Fe"], time_feat_dim=r["Ft"]))


# ---- C: the C contract on hand-built sides ----------------------------------------------------------------------------------------------------
C_MODEL = dict(W=2, k=3, P=24, heads=4, Ft=cc.TIME_FEAT_DIM)
C_PAIRS = (np.array([0, 1, 1, 1, 4, 5], dtype=np.int32),              # (s, s); side 1 with three partners; (a, b) beside (b, a)
           np.array([0, 2, 3, 5, 5, 4], dtype=np.int32))
C_NODE_ROWS, C_EDGE_ROWS = 30, 550                                    # the library's tables in the out-of-range case: the first rows only
C_FAR_NODE, C_FAR_EDGE = 1000, 5000


@functools.lru_cache(maxsize=None)
def c_case() -> dict:
    """Six sides of a 40-node graph, hop arrays edited by hand.  dict(data, node_feat, edge_feat, params, sides, oob_sides,
    oob_sides_restated, node_feat_ext, edge_feat_ext).  Row 0 of both tables is NON-zero: reading row 0 is not reading zeros.  `sides`:
    shared ids put in by hand so that both count rows are non-zero, and one partial tree.  `oob_sides`: node ids at and above C_NODE_ROWS,
    edge ids at and above C_EDGE_ROWS and negative ones; `oob_sides_restated` is the same with edge id 0 where the library gets a negative
    one, for the tables `*_ext`: the first C_NODE_ROWS / C_EDGE_ROWS rows, then copies of row 0."""
    data, nf, ef = syn.make_general_graph(40, 600, seed=23)
    rs = np.random.RandomState(24)
    nf, ef = nf.copy(), ef.copy()
    nf[0], ef[0] = 0.5 * rs.standard_normal(nf.shape[1]), 0.5 * rs.standard_normal(ef.shape[1])
    W, k = C_MODEL["W"], C_MODEL["k"]
    idx = np.array([590, 591, 592])
    roots = np.concatenate([data.src_node_ids[idx], data.dst_node_ids[idx]])
    times = np.concatenate([data.node_interact_times[idx] + 1.0, np.full(3, data.node_interact_times.max() + 1.0)])      # the times of a pair's sides differ
    roots, times, hops = sample_sides(data, W, k, roots, times)
    hops = [(n.copy(), e.copy(), t.copy()) for n, e, t in hops]
    (n1, e1, t1), (n2, e2, t2) = hops
    assert (n1 != 0).all() and (n2 != 0).all()                        # late queries: full trees, every entry may be edited
    n1[2, 2], n2[3, 4], n2[1, 0] = roots[1], roots[1], roots[5]       # a partner's target inside a tree
    n2[4, 8], n2[5, 8] = n1[5, 0], n1[4, 0]
    n1[0, 0] = n2[0, 0] = 0                                           # a partial tree: a padded hop-1 node and its
    n2[0, 1] = n2[0, 2] = 0                                           # three children (zeros are a suffix of a walk)
    e1[0, 0] = e2[0, 0] = e2[0, 1] = e2[0, 2] = 0
    t1[0, 0] = t2[0, 0] = t2[0, 1] = t2[0, 2] = 0.0
    sides = (roots, times, hops)
    on, oe = [h[0].copy() for h in hops], [h[1].copy() for h in hops]
    on[0][1, 1], on[1][1, 3], on[1][2, 5] = C_NODE_ROWS, C_FAR_NODE, C_FAR_NODE      # the first id outside, and one id in both trees of (1, 2)
    on[1][3, 7], on[0][4, 2], on[1][5, 2] = C_NODE_ROWS + 16, C_FAR_NODE, C_FAR_NODE
    oe[0][1, 1], oe[1][1, 3], oe[1][2, 5] = C_EDGE_ROWS, C_FAR_EDGE, -1
    oe[0][3, 0], oe[1][4, 6], oe[1][5, 1] = -7, C_EDGE_ROWS + 5, np.iinfo(np.int64).min
    oob = (roots, times, [(on[h], oe[h], hops[h][2]) for h in range(W)])
    oob_restated = (roots, times, [(on[h], np.where(oe[h] < 0, 0, oe[h]), hops[h][2]) for h in range(W)])
    ext = lambda tab, rows, upto: np.concatenate([tab[:rows], np.repeat(tab[:1], upto + 1 - rows, axis=0)])
    return dict(data=data, node_feat=nf, edge_feat=ef, params=syn.make_cawn_params(PARAM_SEED, C_MODEL["P"], W, C_MODEL["heads"]), sides=sides, oob_sides=oob,
                oob_sides_restated=oob_restated, node_feat_ext=ext(nf, C_NODE_ROWS, C_FAR_NODE), edge_feat_ext=ext(ef, C_EDGE_ROWS, C_FAR_EDGE))


OOB_PAIRS = (np.array([0, 1, 3, 4, 2], dtype=np.int32), np.array([1, 2, 3, 5, 1], dtype=np.int32))
