"""Seeded CAWN recipes shared by tools/make_golden_cawn.py (which runs the reference on them) and by the tests (which rebuild the same inputs
and compare with the stored outputs, tests/golden/cawn_<case>.npz).  Graphs come from tests.golden_cases.build_case, the query batches from
`batch` below, parameters from dyglib_amd.synthetic.make_cawn_params; inputs are never stored."""
from __future__ import annotations

import numpy as np

from dyglib_amd import synthetic as syn
from tests import golden_cases as gc
from tests.graphmixer_cases import node_features

TAP_ROWS = gc.TAP_ROWS
TIME_FEAT_DIM = 100

# name -> graph case, batch (see batch_indices: `head` first edges of the stream among the `tail` last ones or `every` 16th), walk_length W,
# num_neighbors k, position_feat_dim P, heads, param seed, sampling strategy, time_scaling_factor, sampler seed, negative seed
CASES = {
    # M = 5 and B = 37 are multiples of no tile; the first edges of the stream: empty histories on both sides and on one side, walks of
    # length 1 beside full ones; a general graph's two trees share nodes, so both count rows are non-zero
    "gen_w1_k5": dict(graph="gen_p1_l32", head=3, every=34, W=1, k=5, P=172, heads=8, param_seed=601, strategy="recent", scale=0.0, sampler_seed=1,
                      neg_seed=61),
    # the reference's Wikipedia configuration: attention_dim 312, head size 39; the RandomState is consumed call after call
    "bip_w1_k32": dict(graph="bip_p2_l64", head=2, tail=14, W=1, k=32, P=172, heads=8, param_seed=602, strategy="time_interval_aware", scale=1e-6,
                       sampler_seed=5, neg_seed=62),
    # three-position walks, partial walks [t, x, 0], the hub items recur at several hops of both trees, float32 hop-2 query times;
    # D = 468: attention_dim 234 rounded up to 236, head size 59
    "hub_w2_k4": dict(graph="hub_p4_l48", head=1, tail=11, W=2, k=4, P=24, heads=4, param_seed=603, strategy="recent", scale=0.0, sampler_seed=1,
                      neg_seed=63),
    # random draws over two hops, in the reference's order
    "gen_w2_k3_uniform": dict(graph="gen_p1_l32", head=1, every=8, W=2, k=3, P=172, heads=8, param_seed=604, strategy="uniform", scale=0.0,
                              sampler_seed=3, neg_seed=64),
}


def batch_indices(r: dict, E: int) -> np.ndarray:
    """two late interactions, the first `head` edges of the stream, the other late interactions: the first TAP_ROWS pairs hold both kinds"""
    head = np.arange(r["head"])
    late = np.arange(E - r["tail"], E) if "tail" in r else (np.arange(r["every"]) * 16 + 19) % E
    return np.concatenate([late[:2], head, late[2:]])


def history_lengths(data, nodes: np.ndarray, times: np.ndarray) -> np.ndarray:
    """number of interactions of every node strictly before its query time"""
    s, d, t = data.src_node_ids, data.dst_node_ids, data.node_interact_times
    return np.array([int((((s == v) | (d == v)) & (t < tq)).sum()) for v, tq in zip(nodes, times)])


def build_cawn_case(name: str) -> dict:
    """dict(data, node_feat, edge_feat, src, dst, neg_dst, times, cawn_params, cawn_cfg, one_sided): one_sided is the first pair with an
    empty history on exactly one side (None when the batch has none)."""
    r = CASES[name]
    c = gc.build_case(r["graph"])
    data = c["data"]
    idx = batch_indices(r, data.num_interactions)
    src, dst, times = data.src_node_ids[idx].copy(), data.dst_node_ids[idx].copy(), data.node_interact_times[idx].copy()
    neg = syn.random_negative_dst(np.random.RandomState(r["neg_seed"]), np.unique(data.dst_node_ids), len(idx))
    ls, ld = history_lengths(data, src, times), history_lengths(data, dst, times)
    one = np.flatnonzero((ls == 0) != (ld == 0))
    return dict(data=data, node_feat=node_features(c, dict(param_seed=r["param_seed"], row0=False)), edge_feat=c["edge_feat"], src=src, dst=dst,
                neg_dst=neg, times=times, hist_src=ls, hist_dst=ld, one_sided=int(one[0]) if len(one) else None,
                cawn_params=syn.make_cawn_params(r["param_seed"], r["P"], r["W"], r["heads"]),
                cawn_cfg=dict(W=r["W"], k=r["k"], P=r["P"], heads=r["heads"], time_feat_dim=TIME_FEAT_DIM, strategy=r["strategy"], scale=r["scale"],
                              sampler_seed=r["sampler_seed"]))
