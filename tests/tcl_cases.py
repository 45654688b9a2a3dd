"""Seeded TCL recipes shared by tools/make_golden_tcl.py (which runs the reference on them) and by the tests (which rebuild the same inputs
and compare with the stored outputs, tests/golden/tcl_<case>.npz).  Graphs, query batches and negatives come from
tests.golden_cases.build_case; inputs are never stored."""
from __future__ import annotations

from dyglib_amd import synthetic as syn
from tests import golden_cases as gc
from tests.graphmixer_cases import node_features

TAP_ROWS = gc.TAP_ROWS
TIME_FEAT_DIM = 100

# name -> (graph case, num_neighbors K (num_depths = K + 1), num_layers, num_heads, param seed, sampling strategy, sampler seed)
CASES = {
    # 4 source roots without history (sequences that are the root alone), full sequences next to them
    "bip_k20_l2_h2": dict(graph="bip_p2_l64", K=20, layers=2, heads=2, param_seed=501, strategy="recent", sampler_seed=1),
    # general graph: self-loops, duplicate integer times, odd batch 37, one empty source root; one layer: the first layer is the last
    "gen_k5_l1_h2": dict(graph="gen_p1_l32", K=5, layers=1, heads=2, param_seed=502, strategy="recent", sampler_seed=1),
    # 10 of the 24 user roots have no history, hub items have full sequences; head dim 43
    "hub_k10_l3_h4": dict(graph="hub_p4_l48", K=10, layers=3, heads=4, param_seed=503, strategy="recent", sampler_seed=1),
    # random sampling: the sampler's RandomState is consumed source rows first, then destination rows, call after call
    "bip_k20_uniform": dict(graph="bip_p2_l64", K=20, layers=2, heads=2, param_seed=504, strategy="uniform", sampler_seed=3),
}

# evaluation loop fixture (eval_tcl.npz): the eval_tgat recipe's graph and index span, K = 20, batch 40
EVAL = dict(graph="bip_p2_l64", K=20, layers=2, heads=2, param_seed=505, merge_seed=1505, batch=40, strategy="recent", sampler_seed=1)


def build_tcl_case(name: str) -> dict:
    """build_case's dict with node_feat replaced (a bipartite graph's are all zero), plus tcl_params and tcl_cfg."""
    r = CASES[name] if name in CASES else EVAL
    c = gc.build_case(r["graph"])
    c["node_feat"] = node_features(c, dict(param_seed=r["param_seed"], row0=False))
    c["tcl_params"] = syn.make_tcl_params(r["param_seed"], r["K"], num_layers=r["layers"])
    c["tcl_cfg"] = dict(K=r["K"], layers=r["layers"], heads=r["heads"], time_feat_dim=TIME_FEAT_DIM, strategy=r["strategy"],
                        sampler_seed=r["sampler_seed"])
    return c


def build_eval_case() -> dict:
    c = build_tcl_case("eval")
    c["mparams"] = syn.make_merge_layer_params(EVAL["merge_seed"])
    c["tcl_cfg"]["batch"] = EVAL["batch"]
    return c
