"""The CPU restatement tests/tcl_oracle.py against the reference's own outputs (tests/golden/tcl_<case>.npz, written by
tools/make_golden_tcl.py): the embeddings of the (src, dst) call and of the (src, neg_dst) call, and the taps of the first TAP_ROWS pairs at
the valid (not padded) positions, under the plain 1e-4 bar."""
import numpy as np
import pytest

from oracle import dygformer_oracle as orc
from tests import golden_cases as gc
from tests import parity
from tests import tcl_cases as tc
from tests import tcl_oracle as tco


def check_taps(name, taps, g, what="tcl"):
    """encoder input and layer outputs [r, 2, S, d] against the fixture where the fixture's node ids are non-zero"""
    ok = tco.valid(g["tap_ids"])
    assert ok[:, :, 0].all()                             # position 0 is the root: always valid
    parity.close(np.asarray(taps["encoder_input"])[ok], g["tap_encoder_input"][ok], f"{name} encoder input", f"{what} encoder input")
    for l, x in enumerate(taps["layer_out"]):
        parity.close(np.asarray(x)[ok], g[f"tap_layer_out_{l}"][ok], f"{name} layer {l}", f"{what} layer output")


class OracleSampler:
    """the reference's sampler calls, restated: `recent`, or `uniform` on one RandomState that carries over from call to call"""

    def __init__(self, data, strategy, seed):
        self.adj = orc.OracleAdjacency(data.src_node_ids, data.dst_node_ids, data.edge_ids, data.node_interact_times)
        self.strategy, self.seed = strategy, seed
        self.reset()

    def reset(self):
        self.rs = np.random.RandomState(self.seed)

    def __call__(self, ids, times, k):
        if self.strategy == "recent":
            return orc.get_historical_neighbors_recent(self.adj, ids, times, k)
        return tco.sample_uniform(self.adj, ids, times, k, self.rs)


def oracle_call(c, smp, src, dst, times, taps=False):
    cfg = c["tcl_cfg"]
    a = smp(src, times, cfg["K"])                       # sources first, then destinations (models/TCL.py:70-82)
    b = smp(dst, times, cfg["K"])
    return tco.tcl_forward(c["tcl_params"], c["node_feat"], c["edge_feat"], src, dst, times, a, b, cfg["layers"], cfg["heads"], taps=taps)


@pytest.mark.parametrize("name", list(tc.CASES))
def test_restatement_matches_reference(name):
    c = tc.build_tcl_case(name)
    g = gc.load_golden(f"tcl_{name}")
    cfg = c["tcl_cfg"]
    smp = OracleSampler(c["data"], cfg["strategy"], cfg["sampler_seed"])
    s, d = oracle_call(c, smp, c["src"], c["dst"], c["times"])
    sn, nd = oracle_call(c, smp, c["src"], c["neg_dst"], c["times"])
    for got, key in ((s, "src_emb"), (d, "dst_emb"), (sn, "src_neg_emb"), (nd, "neg_dst_emb")):
        parity.close(got, g[key], f"{name} {key}", "tcl oracle embeddings")
    r = min(tc.TAP_ROWS, len(c["src"]))
    smp.reset()
    _, _, taps = oracle_call(c, smp, c["src"][:r], c["dst"][:r], c["times"][:r], taps=True)
    assert np.array_equal(taps["ids"], g["tap_ids"])
    check_taps(name, taps, g, "tcl oracle")


def test_fixture_recipes_exercise_what_they_claim():
    """empty-history source roots, the partner dependence of the source embedding, padded tap positions and head dim 43"""
    want_empty = {"bip_k20_l2_h2": 4, "gen_k5_l1_h2": 1, "hub_k10_l3_h4": 10}
    for name, n in want_empty.items():
        c = tc.build_tcl_case(name)
        d = c["data"]
        adj = orc.OracleAdjacency(d.src_node_ids, d.dst_node_ids, d.edge_ids, d.node_interact_times)
        lens = np.array([len(orc.find_neighbors_before(adj, v, t)[0]) for v, t in zip(c["src"], c["times"])])
        assert int((lens == 0).sum()) == n, (name, int((lens == 0).sum()))
        g = gc.load_golden(f"tcl_{name}")
        assert 0.3 < np.abs(g["src_emb"] - g["src_neg_emb"]).max() < 1.0
    assert not tco.valid(gc.load_golden("tcl_bip_k20_l2_h2")["tap_ids"]).all()
    assert 172 // tc.CASES["hub_k10_l3_h4"]["heads"] == 43 and len(c["src"]) == 24 and len(tc.build_tcl_case("gen_k5_l1_h2")["src"]) == 37
