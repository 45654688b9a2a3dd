"""dyglib_amd.CAWN (dygnn_cawn_forward, dyglib_amd/csrc/cawn.hip) on an MI355X against the reference's own outputs
(tests/golden/cawn_<case>.npz) on every fixture case: the embeddings of the (src, dst) and the (src, neg_dst) call on ONE sampler, the taps
of the first TAP_ROWS pairs, compute_step_embeddings, a single-pair call, train mode under no_grad, and the refusals.  Plain absolute 1e-4
(tests/parity.py) on embeddings and float taps, walk ids exact, position counts 1e-5 (tests/test_cawn_cpu.py derives the bound)."""
import functools

import numpy as np
import pytest

from tests import cawn_cases as cc
from tests import golden_cases as gc
from tests import parity
from tests.test_cawn_cpu import EMB_KEYS, check_taps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def case_model(name):
    import torch
    from dyglib_amd import CAWN, get_neighbor_sampler
    c = cc.build_cawn_case(name)
    cfg = c["cawn_cfg"]
    sampler = get_neighbor_sampler(c["data"], cfg["strategy"], time_scaling_factor=cfg["scale"], seed=cfg["sampler_seed"], device=DEV)
    m = CAWN(c["node_feat"], c["edge_feat"], sampler, cc.TIME_FEAT_DIM, cfg["P"], walk_length=cfg["W"], num_walk_heads=cfg["heads"], dropout=0.1, device=DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["cawn_params"].items()}, strict=True)
    return c, cfg, m.to(DEV).eval(), gc.load_golden(f"cawn_{name}")


@pytest.mark.parametrize("name", list(cc.CASES))
def test_fixture_case_matches_reference(name):
    import torch
    c, cfg, m, g = case_model(name)
    k = cfg["k"]
    r = min(cc.TAP_ROWS, len(c["src"]))
    with torch.no_grad():
        m.set_neighbor_sampler(m.neighbor_sampler)
        got = m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=k)
        got += m.compute_src_dst_node_temporal_embeddings(c["src"], c["neg_dst"], c["times"], num_neighbors=k)
        m.set_neighbor_sampler(m.neighbor_sampler)                   # resets a random sampler's state, as the fixture's tap call did
        ts, td, taps = m.compute_src_dst_node_temporal_embeddings(c["src"][:r], c["dst"][:r], c["times"][:r], num_neighbors=k, taps=r)
    for x, key in zip(got, EMB_KEYS):
        parity.close(x.cpu().numpy(), g[key], f"{name} {key}", "cawn embeddings vs reference")
    if cfg["strategy"] == "recent":                                  # a pair's rows do not depend on the other pairs, nor on the taps
        assert torch.equal(ts, got[0][:r]) and torch.equal(td, got[1][:r])
    check_taps(name + " (gpu)", {k_: v.cpu().numpy() for k_, v in taps.items()}, g, "cawn")


@pytest.mark.parametrize("name", list(cc.CASES))
def test_step_embeddings_match_reference(name):
    import torch
    c, cfg, m, g = case_model(name)
    with torch.no_grad():
        m.set_neighbor_sampler(m.neighbor_sampler)
        step = m.compute_step_embeddings(c["src"], c["dst"], c["neg_dst"], c["times"], num_neighbors=cfg["k"])
    assert len(step) == 4
    for x, key in zip(step, EMB_KEYS):
        parity.close(x.cpu().numpy(), g[key], f"{name} step {key}", "cawn step embeddings vs reference")
    assert not torch.equal(step[0], step[2])                         # the source embedding depends on its partner


@pytest.mark.parametrize("name", [n for n, r in cc.CASES.items() if r["strategy"] == "recent"])
def test_single_pair_with_an_empty_history_on_one_side(name):
    import torch
    c, cfg, m, g = case_model(name)
    i = c["one_sided"]
    assert i is not None and (c["hist_src"][i] == 0) != (c["hist_dst"][i] == 0)
    with torch.no_grad():
        s, d = m.compute_src_dst_node_temporal_embeddings(c["src"][i:i + 1], c["dst"][i:i + 1], c["times"][i:i + 1], num_neighbors=cfg["k"])
    parity.close(s.cpu().numpy(), g["src_emb"][i:i + 1], f"{name} pair {i} alone, src", "cawn embeddings vs reference")
    parity.close(d.cpu().numpy(), g["dst_emb"][i:i + 1], f"{name} pair {i} alone, dst", "cawn embeddings vs reference")


@pytest.mark.parametrize("name", list(cc.CASES))
def test_train_mode_under_no_grad_equals_eval_mode(name):
    import torch
    c, cfg, m, g = case_model(name)
    a = (c["src"], c["dst"], c["times"])
    try:
        with torch.no_grad():
            m.set_neighbor_sampler(m.neighbor_sampler)
            ev = m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=cfg["k"])
            m.train()
            m.set_neighbor_sampler(m.neighbor_sampler)
            tr = m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=cfg["k"])
        with pytest.raises(NotImplementedError, match="inference-only"):
            m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=cfg["k"])
    finally:
        m.eval()
    assert torch.equal(ev[0], tr[0]) and torch.equal(ev[1], tr[1])
    with pytest.raises(NotImplementedError, match="inference-only"):                  # eval mode, autograd recording
        m.compute_step_embeddings(c["src"], c["dst"], c["neg_dst"], c["times"], num_neighbors=cfg["k"])


def test_empty_batch_and_bad_arguments_raise_before_any_launch():
    import torch
    from dyglib_amd import CAWN
    c, cfg, m, g = case_model("gen_w1_k5")
    with torch.no_grad():
        s, d = m.compute_src_dst_node_temporal_embeddings(c["src"][:0], c["dst"][:0], c["times"][:0], num_neighbors=5)
        assert s.shape == d.shape == (0, 172) and s.device.type == "cuda"
        assert all(x.shape == (0, 172) for x in m.compute_step_embeddings(c["src"][:0], c["dst"][:0], c["neg_dst"][:0], c["times"][:0], num_neighbors=5))
        with pytest.raises(IndexError):
            m.compute_src_dst_node_temporal_embeddings(np.array([10 ** 6]), np.array([1]), np.array([1.0]), num_neighbors=5)
        with pytest.raises(AssertionError, match="padding node"):
            m.compute_src_dst_node_temporal_embeddings(np.array([0]), np.array([1]), np.array([1.0]), num_neighbors=5)
        with pytest.raises(AssertionError, match="greater than 0"):
            m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=0)
        with pytest.raises(NotImplementedError, match=r"129 walks \(num_neighbors 129 \*\* walk_length 1\) > 128 not supported"):
            m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=129)
        wide = CAWN(np.zeros((c["node_feat"].shape[0], 260), np.float32), c["edge_feat"], m.neighbor_sampler, cc.TIME_FEAT_DIM, 172, walk_length=1,
                    device=DEV).to(DEV).eval()
        with pytest.raises(NotImplementedError, match="node_feat_dim 260 > 256 not supported"):
            wide.compute_src_dst_node_temporal_embeddings(np.array([1]), np.array([2]), np.array([5.0]), num_neighbors=4)
        deep = CAWN(c["node_feat"], c["edge_feat"], m.neighbor_sampler, cc.TIME_FEAT_DIM, 24, walk_length=3, num_walk_heads=4, device=DEV).to(DEV).eval()
        with pytest.raises(NotImplementedError, match="walk_length 3 not supported"):
            deep.compute_src_dst_node_temporal_embeddings(np.array([1]), np.array([2]), np.array([5.0]), num_neighbors=2)


def against_restatement(W, k, P, heads, Fn=172, n=5, what=""):
    """shapes without a fixture: against tests/cawn_oracle.py (itself pinned to the fixtures) on hops sampled by the package's sampler"""
    import torch
    from dyglib_amd import CAWN, get_neighbor_sampler, synthetic as syn
    from tests import cawn_oracle as cwo
    data, nf, ef = syn.make_bipartite_graph(60, 9, 6000, seed=3, duplicate_time_every=5)
    rs = np.random.RandomState(4)
    nf = (0.5 * rs.standard_normal((nf.shape[0], Fn))).astype(np.float32)
    nf[0] = 0.0
    params = syn.make_cawn_params(5, P, W, heads, node_feat_dim=Fn)
    sampler = get_neighbor_sampler(data, "recent", seed=1, device=DEV)
    m = CAWN(nf, ef, sampler, cc.TIME_FEAT_DIM, P, walk_length=W, num_walk_heads=heads, device=DEV)
    m.load_state_dict({k_: torch.from_numpy(v) for k_, v in params.items()}, strict=True)
    m = m.to(DEV).eval()
    idx = rs.randint(0, data.num_interactions, n)
    src, dst = data.src_node_ids[idx].astype(np.int64), data.dst_node_ids[idx].astype(np.int64)
    times = data.node_interact_times[idx].astype(np.float64)
    times[0] = data.node_interact_times.min() - 1.0                  # both histories empty
    with torch.no_grad():
        s, d = m.compute_src_dst_node_temporal_embeddings(src, dst, times, num_neighbors=k)
    a, b = sampler.get_multi_hop_neighbors(W, src, times, k), sampler.get_multi_hop_neighbors(W, dst, times, k)
    ws, wd = cwo.cawn_forward(params, nf, ef, src, dst, times, a, b, heads)
    parity.close(s.cpu().numpy(), ws, f"cawn {what} src", "cawn embeddings vs restatement")
    parity.close(d.cpu().numpy(), wd, f"cawn {what} dst", "cawn embeddings vs restatement")


def test_attention_dim_above_320():
    against_restatement(1, 5, 172, 8, Fn=256, what="attention_dim 352")        # eight column tiles per wave, 32-row tiles; hidden 350


def test_more_than_64_walks():
    against_restatement(2, 9, 24, 4, what="W=2 k=9, 81 walks")                 # two keys per lane in the attention, tree of 91 positions


def test_128_walks_and_one_neighbour():
    against_restatement(1, 128, 24, 4, n=3, what="W=1 k=128")                  # the largest tree: 129 positions, 258 hash keys
    against_restatement(2, 1, 24, 4, n=3, what="W=2 k=1")                      # one walk: softmax over a single key


def test_position_feat_dim_two_mod_four():
    against_restatement(1, 5, 170, 8, what="P=170")                            # D = 614: weight rows 8-byte aligned, hidden sizes 307 and 85
    against_restatement(2, 3, 6, 4, what="W=2 k=3 P=6")                        # position encoder with hidden size 3
