"""The CPU restatement tests/graphmixer_oracle.py against the reference's own outputs (tests/golden/graphmixer_<case>.npz, written by
tools/make_golden_graphmixer.py): embeddings of every root and the taps of the first TAP_ROWS source roots under the plain 1e-4 bar.

The node-encoder term is O(1 / time_gap) (about 6e-4 at time_gap 2000), so an absolute 1e-4 on it would prove nothing: it is compared as
time_gap * term, the plain mean of the valid neighbour rows, O(1), under the same bar.  An fp32 sequential row sum differs from the reference by
<= 6.2e-7 on that quantity at m = 2000, so the bar has two orders of margin and still catches a dropped row, a wrong m or a missing 1 / G."""
import numpy as np
import pytest

from oracle import dygformer_oracle as orc
from tests import golden_cases as gc
from tests import graphmixer_cases as gmc
from tests import graphmixer_oracle as gmo
from tests import parity


def check_taps(name, taps, g, G, rows):
    parity.close(np.asarray(taps["projection"])[:rows], g["tap_projection"], f"{name} projection", "graphmixer projection")
    for l, x in enumerate(taps["layer_out"]):
        parity.close(np.asarray(x)[:rows], g[f"tap_layer_out_{l}"], f"{name} mixer block {l}", "graphmixer mixer block output")
    parity.close(np.asarray(taps["token_mean"])[:rows], g["tap_token_mean"], f"{name} token mean", "graphmixer token mean")
    parity.close(G * np.asarray(taps["node_term"], dtype=np.float64)[:rows], G * g["tap_node_term"].astype(np.float64),
                 f"{name} time_gap * node term", "graphmixer time_gap * node term")


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("name", list(gmc.CASES))
def test_restatement_matches_reference(name, dense):
    c = gmc.build_graphmixer_case(name)
    g = gc.load_golden(f"graphmixer_{name}")
    cfg = c["gm_cfg"]
    d = c["data"]
    adj = orc.OracleAdjacency(d.src_node_ids, d.dst_node_ids, d.edge_ids, d.node_interact_times)
    B = len(c["src"])
    roots = np.concatenate([c["src"], c["dst"], c["neg_dst"]])
    emb, taps = gmo.graphmixer_forward(c["gm_params"], c["node_feat"], c["edge_feat"], adj, roots, np.tile(c["times"], 3), cfg["K"], cfg["G"],
                                       cfg["layers"], taps=True, dense_node_term=dense)
    for part, key in enumerate(("src_emb", "dst_emb", "neg_dst_emb")):
        parity.close(emb[part * B:(part + 1) * B], g[key], f"{name} {key}", "graphmixer oracle embeddings")
    check_taps(name, taps, g, cfg["G"], min(gmc.TAP_ROWS, B))


def test_fixture_recipes_exercise_what_they_claim():
    """empty histories, windows truncated at time_gap and the non-zero padding row are present in the recipes"""
    seen_empty = seen_trunc = seen_row0 = False
    for name in gmc.CASES:
        c = gmc.build_graphmixer_case(name)
        d = c["data"]
        adj = orc.OracleAdjacency(d.src_node_ids, d.dst_node_ids, d.edge_ids, d.node_interact_times)
        lens = np.array([len(orc.find_neighbors_before(adj, v, t)[0]) for v, t in zip(np.concatenate([c["src"], c["dst"]]), np.tile(c["times"], 2))])
        seen_empty |= bool((lens == 0).any())
        seen_trunc |= bool((lens > c["gm_cfg"]["G"]).any())
        seen_row0 |= bool(c["node_feat"][0].any() and (lens == 0).any())
    assert seen_empty and seen_trunc and seen_row0
