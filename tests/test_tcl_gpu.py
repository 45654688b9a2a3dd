"""dyglib_amd.TCL (dygnn_tcl_forward, dyglib_amd/csrc/tcl.hip) on an MI355X: against the reference's own outputs (tests/golden/tcl_<case>.npz)
on every fixture case, and against the CPU restatement (tests/tcl_oracle.py, itself pinned to the fixtures) at shapes that have none.  Plain
absolute 1e-4 (tests/parity.py) on every embedding and on the taps at valid positions."""
import numpy as np
import pytest

from dyglib_amd import synthetic as syn
from tests import golden_cases as gc
from tests import parity
from tests import tcl_cases as tc
from tests import tcl_oracle as tco
from tests.test_tcl_oracle_golden import check_taps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make_model(node_feat, edge_feat, data, params, K, layers, heads, time_feat_dim=100, strategy="recent", seed=1, scale=0.0):
    import torch
    from dyglib_amd import TCL, get_neighbor_sampler
    sampler = get_neighbor_sampler(data, strategy, time_scaling_factor=scale, seed=seed, device=DEV)
    m = TCL(node_feat, edge_feat, sampler, time_feat_dim, num_layers=layers, num_heads=heads, num_depths=K + 1, dropout=0.1, device=DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return m.to(DEV).eval()


def case_model(name):
    c = tc.build_tcl_case(name)
    cfg = c["tcl_cfg"]
    m = make_model(c["node_feat"], c["edge_feat"], c["data"], c["tcl_params"], cfg["K"], cfg["layers"], cfg["heads"], strategy=cfg["strategy"],
                   seed=cfg["sampler_seed"])
    return c, cfg, m


@pytest.mark.parametrize("name", list(tc.CASES))
def test_fixture_case_matches_reference(name):
    import torch
    c, cfg, m = case_model(name)
    g = gc.load_golden(f"tcl_{name}")
    K = cfg["K"]
    r = min(tc.TAP_ROWS, len(c["src"]))
    with torch.no_grad():
        m.set_neighbor_sampler(m.neighbor_sampler)
        s, d = m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=K)
        sn, nd = m.compute_src_dst_node_temporal_embeddings(c["src"], c["neg_dst"], c["times"], num_neighbors=K)
        m.set_neighbor_sampler(m.neighbor_sampler)                   # resets a random sampler's state, as the fixture's tap call did
        ts, td, taps = m.compute_src_dst_node_temporal_embeddings(c["src"][:r], c["dst"][:r], c["times"][:r], num_neighbors=K, taps=r)
    for got, key in ((s, "src_emb"), (d, "dst_emb"), (sn, "src_neg_emb"), (nd, "neg_dst_emb")):
        parity.close(got.cpu().numpy(), g[key], f"{name} {key}", "tcl embeddings vs reference")
    if cfg["strategy"] == "recent":                                  # with taps the last layer is computed at every position: position 0 must not change
        assert torch.equal(ts, s[:r]) and torch.equal(td, d[:r])
    taps = dict(encoder_input=taps["encoder_input"].cpu().numpy(), layer_out=[x.cpu().numpy() for x in taps["layer_out"]])
    check_taps(name + " (gpu)", taps, g, "tcl")


@pytest.mark.parametrize("name", list(tc.CASES))
def test_entry_points_agree_bit_for_bit(name):
    """a pair's rows do not depend on what else is in the call, nor on how the call was made"""
    import torch
    c, cfg, m = case_model(name)
    K = cfg["K"]
    src, dst, neg, t = c["src"], c["dst"], c["neg_dst"], c["times"]
    with torch.no_grad():
        m.set_neighbor_sampler(m.neighbor_sampler)
        s, d = m.compute_src_dst_node_temporal_embeddings(src, dst, t, num_neighbors=K)
        sn, nd = m.compute_src_dst_node_temporal_embeddings(src, neg, t, num_neighbors=K)
        m.set_neighbor_sampler(m.neighbor_sampler)
        step = m.compute_step_embeddings(src, dst, neg, t, num_neighbors=K)
    for a, b in zip(step, (s, d, sn, nd)):
        assert torch.equal(a, b)
    assert not torch.equal(s, sn)                                    # the source embedding depends on its partner
    if cfg["strategy"] != "recent":
        return                                                       # the draws of a random sampler depend on the batch
    with torch.no_grad():
        one = m.compute_src_dst_node_temporal_embeddings(src[5:6], dst[5:6], t[5:6], num_neighbors=K)
        rev = m.compute_src_dst_node_temporal_embeddings(src[::-1].copy(), dst[::-1].copy(), t[::-1].copy(), num_neighbors=K)
        to = lambda x, dt: torch.from_numpy(x).to(device=DEV, dtype=dt)
        ten = m.compute_src_dst_node_temporal_embeddings(to(src, torch.int64), to(dst, torch.int64), to(t, torch.float64), num_neighbors=K)
        st = torch.cuda.Stream(device=DEV)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            on_stream = m.compute_src_dst_node_temporal_embeddings(src, dst, t, num_neighbors=K)
            step_stream = m.compute_step_embeddings(src, dst, neg, t, num_neighbors=K)
        st.synchronize()
    assert torch.equal(one[0][0], s[5]) and torch.equal(one[1][0], d[5])
    assert torch.equal(rev[0].flip(0), s) and torch.equal(rev[1].flip(0), d)
    assert torch.equal(ten[0], s) and torch.equal(ten[1], d)
    assert torch.equal(on_stream[0], s) and torch.equal(on_stream[1], d) and torch.equal(step_stream[2], sn) and torch.equal(step_stream[3], nd)


def synthetic_setup(K, layers, dims=None, seed=3):
    """a bipartite graph with non-zero node features and seeded parameters"""
    Fn, Fe, Ft = (172, 172, 100) if dims is None else dims
    data, nf, ef = syn.make_bipartite_graph(60, 9, 6000, seed=seed, duplicate_time_every=5)
    rs = np.random.RandomState(seed + 1)
    nf = (0.5 * rs.standard_normal((nf.shape[0], Fn))).astype(np.float32)
    nf[0] = 0.0
    ef = np.ascontiguousarray(ef[:, :Fe])
    params = syn.make_tcl_params(seed + 2, K, num_layers=layers, node_feat_dim=Fn, edge_feat_dim=Fe, time_feat_dim=Ft)
    return data, nf, ef, params, Ft


def pairs_of(data, n, seed, all_empty=False):
    """n interactions as (src, dst, time): histories of every length; the first precedes every interaction (both histories empty)"""
    rs = np.random.RandomState(seed)
    idx = rs.randint(0, data.num_interactions, n)
    src, dst = data.src_node_ids[idx].astype(np.int64), data.dst_node_ids[idx].astype(np.int64)
    times = data.node_interact_times[idx].astype(np.float64)
    times[0] = data.node_interact_times.min() - 1.0
    if all_empty:
        times[:] = data.node_interact_times.min() - 1.0
    return src, dst, times


def against_oracle(K, layers, heads, n, dims=None, strategy="recent", scale=0.0, all_empty=False, what=""):
    import torch
    from dyglib_amd import get_neighbor_sampler
    data, nf, ef, params, Ft = synthetic_setup(K, layers, dims)
    m = make_model(nf, ef, data, params, K, layers, heads, Ft, strategy=strategy, seed=9, scale=scale)
    src, dst, times = pairs_of(data, n, 100 + n, all_empty)
    with torch.no_grad():
        m.set_neighbor_sampler(m.neighbor_sampler)
        s, d = m.compute_src_dst_node_temporal_embeddings(src, dst, times, num_neighbors=K)
    twin = get_neighbor_sampler(data, strategy, time_scaling_factor=scale, seed=9, device=DEV)      # bit-exact with the reference's sampler
    a = twin.get_historical_neighbors(src, times, K)
    b = twin.get_historical_neighbors(dst, times, K)
    if all_empty:
        assert not a[0].any() and not b[0].any()
    ws, wd = tco.tcl_forward(params, nf, ef, src, dst, times, a, b, layers, heads)
    label = f"tcl {what} K={K} L={layers} H={heads} n={n}"
    parity.close(s.cpu().numpy(), ws, label + " src", "tcl embeddings vs restatement")
    parity.close(d.cpu().numpy(), wd, label + " dst", "tcl embeddings vs restatement")


@pytest.mark.parametrize("K", [1, 7, 32, 63])
def test_neighbor_counts(K):
    against_oracle(K, 2, 2, 37)            # S = 2, 8, 33, 64: one to four row tiles, the last one partly filled


@pytest.mark.parametrize("n", [1, 1537])
def test_pair_counts(n):
    against_oracle(7, 2, 2, n)             # 1537 pairs: 3074 sequences of 8 rows, a multiple of no tile (16 rows, 64 token rows)


@pytest.mark.parametrize("heads", [1, 2, 8])
def test_small_dims(heads):
    against_oracle(4, 2, heads, 45, dims=(16, 16, 16), what="dims=(16, 16, 16)")


def test_unequal_dims():
    against_oracle(4, 2, 2, 45, dims=(32, 16, 16), what="dims=(32, 16, 16)")


def test_max_layers():
    from dyglib_amd import _capi
    against_oracle(4, _capi.DYGNN_MAX_LAYERS, 2, 21)


def test_every_root_without_history():
    against_oracle(10, 2, 2, 19, all_empty=True, what="empty histories")


def test_time_interval_aware_sampler():
    against_oracle(10, 2, 2, 41, strategy="time_interval_aware", scale=1e-6, what="time_interval_aware")


def test_empty_batch_and_bad_arguments_raise_before_any_launch():
    import torch
    c, cfg, m = case_model("gen_k5_l1_h2")
    a = (c["src"], c["dst"], c["times"])
    with torch.no_grad():
        s, d = m.compute_src_dst_node_temporal_embeddings(c["src"][:0], c["dst"][:0], c["times"][:0], num_neighbors=5)
        assert s.shape == d.shape == (0, 172)
        assert all(x.shape == (0, 172) for x in m.compute_step_embeddings(c["src"][:0], c["dst"][:0], c["neg_dst"][:0], c["times"][:0], num_neighbors=5))
        with pytest.raises(AssertionError, match="greater than 0"):
            m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=0)
        with pytest.raises(AssertionError, match="num_depths"):
            m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=20)
        with pytest.raises(IndexError):
            m.compute_src_dst_node_temporal_embeddings(np.array([10 ** 6]), np.array([1]), np.array([1.0]), num_neighbors=5)
        with pytest.raises(AssertionError, match="padding node"):
            m.compute_src_dst_node_temporal_embeddings(np.array([0]), np.array([1]), np.array([1.0]), num_neighbors=5)
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=5)
    m.train()
    with torch.no_grad():                                   # train mode without recording is the same forward (dropout is the training PR's)
        s, _ = m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=5)
    parity.close(s.cpu().numpy(), gc.load_golden("tcl_gen_k5_l1_h2")["src_emb"], "train mode, no_grad", "tcl embeddings vs reference")
    data, nf, ef, params, Ft = synthetic_setup(4, 1)
    from dyglib_amd import TCL, get_neighbor_sampler
    wide = TCL(np.zeros((nf.shape[0], 260), np.float32), ef, get_neighbor_sampler(data, "recent", seed=1, device=DEV), Ft, num_layers=1, num_heads=2,
               num_depths=5, device=DEV).to(DEV).eval()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="node_feat_dim 260 > 256"):
        wide.compute_src_dst_node_temporal_embeddings(np.array([1]), np.array([2]), np.array([5.0]), num_neighbors=4)
    long = TCL(nf, ef, get_neighbor_sampler(data, "recent", seed=1, device=DEV), Ft, num_layers=1, num_heads=2, num_depths=65, device=DEV).to(DEV).eval()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="num_neighbors 64 not supported"):
        long.compute_src_dst_node_temporal_embeddings(np.array([1]), np.array([2]), np.array([5.0]), num_neighbors=64)
