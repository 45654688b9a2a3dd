"""Seeded GraphMixer recipes shared by tools/make_golden_graphmixer.py (which runs the reference on them) and by the tests (which rebuild the
same inputs and compare with the stored outputs, tests/golden/graphmixer_<case>.npz).  Graphs, query batches and negatives come from
tests.golden_cases.build_case; inputs are never stored."""
from __future__ import annotations

import numpy as np

from dyglib_amd import synthetic as syn
from tests import golden_cases as gc

TAP_ROWS = gc.TAP_ROWS
TIME_FEAT_DIM = 100

# name -> (graph case, num_neighbors = num_tokens K, num_layers, time_gap G, param seed, node-feature row 0 non-zero)
CASES = {
    # m (neighbours the node encoder reads) from 0 to 411, 7 empty-history roots among [src ; dst]
    "bip_k30_g2000": dict(graph="bip_p2_l64", K=30, layers=2, G=2000, param_seed=401, row0=False),
    # 48 resp. 69 of the 80 [src ; dst] roots are truncated at G; row 0 non-zero in the G = 7 recipe: pins the m = 0 branch (node_feat[0] / G)
    "bip_k30_g50": dict(graph="bip_p2_l64", K=30, layers=2, G=50, param_seed=401, row0=False),
    "bip_k30_g7_row0": dict(graph="bip_p2_l64", K=30, layers=2, G=7, param_seed=401, row0=True),
    # general graph: self-loops, duplicate integer times, odd batch 37, 2 empty roots; one Mixer block
    "gen_k10_g2000": dict(graph="gen_p1_l32", K=10, layers=1, G=2000, param_seed=402, row0=False),
    "gen_k10_g7": dict(graph="gen_p1_l32", K=10, layers=1, G=7, param_seed=402, row0=False),
    # degrees 2250 .. 3000: m = G = 2000 on 10 of the 12 [src ; dst] roots, the full-length walk
    "long_k20_g2000": dict(graph="bip_p64_l2048", K=20, layers=2, G=2000, param_seed=403, row0=False),
    # the 24 user roots have 0 .. 3 neighbours (10 none: token tiles that are all or almost all padding) next to 24 hub roots with 30 filled slots
    "hub_k30_l3_g2000": dict(graph="hub_p4_l48", K=30, layers=3, G=2000, param_seed=404, row0=False),
}

# evaluation loop fixture (eval_graphmixer.npz): the eval_tgat recipe's graph and index span, K = 30, G = 2000, batch 40
EVAL = dict(graph="bip_p2_l64", K=30, layers=2, G=2000, param_seed=405, merge_seed=1405, batch=40)


def node_features(case: dict, recipe: dict) -> np.ndarray:
    """The graph's node features, or for a bipartite graph (all zero there) seeded 0.5 N(0, 1) rows as build_tgn_case makes them; row 0
    (the padding node) stays zero unless the recipe asks otherwise."""
    nf = case["node_feat"].copy()
    if not nf.any():
        rs = np.random.RandomState(recipe["param_seed"] + 7)
        nf[1:] = 0.5 * rs.standard_normal(nf[1:].shape).astype(np.float32)
        if recipe["row0"]:
            nf[0] = 0.5 * rs.standard_normal(nf[0].shape).astype(np.float32)
    return nf


def build_graphmixer_case(name: str) -> dict:
    """build_case's dict with node_feat replaced, plus gm_params and gm_cfg(K, layers, G, time_feat_dim)."""
    r = CASES[name]
    c = gc.build_case(r["graph"])
    c["node_feat"] = node_features(c, r)
    c["gm_params"] = syn.make_graphmixer_params(r["param_seed"], r["K"], num_layers=r["layers"])
    c["gm_cfg"] = dict(K=r["K"], layers=r["layers"], G=r["G"], time_feat_dim=TIME_FEAT_DIM)
    return c


def build_eval_case() -> dict:
    r = dict(EVAL, row0=False)
    c = gc.build_case(r["graph"])
    c["node_feat"] = node_features(c, r)
    c["gm_params"] = syn.make_graphmixer_params(r["param_seed"], r["K"], num_layers=r["layers"])
    c["mparams"] = syn.make_merge_layer_params(r["merge_seed"])
    c["gm_cfg"] = dict(K=r["K"], layers=r["layers"], G=r["G"], time_feat_dim=TIME_FEAT_DIM, batch=r["batch"])
    return c
