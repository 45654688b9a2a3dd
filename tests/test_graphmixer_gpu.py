"""dyglib_amd.GraphMixer (dygnn_graphmixer_forward, dyglib_amd/csrc/graphmixer.hip) on an MI355X: against the reference's own outputs
(tests/golden/graphmixer_<case>.npz) on every fixture case, and against the CPU restatement (tests/graphmixer_oracle.py, itself pinned to the
fixtures) at shapes that have none.  Plain absolute 1e-4 (tests/parity.py) on every root; the node-encoder term is compared scaled by
time_gap (see tests/test_graphmixer_oracle_golden.py)."""
import numpy as np
import pytest

from dyglib_amd import synthetic as syn
from oracle import dygformer_oracle as orc
from tests import golden_cases as gc
from tests import graphmixer_cases as gmc
from tests import graphmixer_oracle as gmo
from tests import parity
from tests.test_graphmixer_oracle_golden import check_taps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make_model(node_feat, edge_feat, data, params, K, layers, time_feat_dim=100):
    import torch
    from dyglib_amd import GraphMixer, get_neighbor_sampler
    sampler = get_neighbor_sampler(data, "recent", seed=1, device=DEV)
    m = GraphMixer(node_feat, edge_feat, sampler, time_feat_dim, num_tokens=K, num_layers=layers, dropout=0.1, device=DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return m.to(DEV).eval()


def case_model(name):
    c = gmc.build_graphmixer_case(name)
    cfg = c["gm_cfg"]
    return c, cfg, make_model(c["node_feat"], c["edge_feat"], c["data"], c["gm_params"], cfg["K"], cfg["layers"])


def adjacency(data):
    return orc.OracleAdjacency(data.src_node_ids, data.dst_node_ids, data.edge_ids, data.node_interact_times)


@pytest.mark.parametrize("name", list(gmc.CASES))
def test_fixture_case_matches_reference(name):
    import torch
    c, cfg, m = case_model(name)
    g = gc.load_golden(f"graphmixer_{name}")
    K, G = cfg["K"], cfg["G"]
    with torch.no_grad():
        s, d = m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=K, time_gap=G)
        s2, nd = m.compute_src_dst_node_temporal_embeddings(c["src"], c["neg_dst"], c["times"], num_neighbors=K, time_gap=G)
        r = min(gmc.TAP_ROWS, len(c["src"]))
        e, taps = m.compute_node_temporal_embeddings(c["src"], c["times"], num_neighbors=K, time_gap=G, taps=r)
    for got, key in ((s, "src_emb"), (d, "dst_emb"), (nd, "neg_dst_emb"), (s2, "src_emb"), (e, "src_emb")):
        parity.close(got.cpu().numpy(), g[key], f"{name} {key}", "graphmixer embeddings vs reference")
    taps = {k: ([x.cpu().numpy() for x in v] if isinstance(v, list) else v.cpu().numpy()) for k, v in taps.items()}
    check_taps(name + " (gpu)", taps, g, G, r)


@pytest.mark.parametrize("name", ["bip_k30_g50", "gen_k10_g7", "hub_k30_l3_g2000"])
def test_entry_points_agree_bit_for_bit(name):
    """a root's row does not depend on what else is in the call"""
    import torch
    c, cfg, m = case_model(name)
    kw = dict(num_neighbors=cfg["K"], time_gap=cfg["G"])
    with torch.no_grad():
        s, d = m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], **kw)
        _, nd = m.compute_src_dst_node_temporal_embeddings(c["src"], c["neg_dst"], c["times"], **kw)
        s3, d3, n3 = m.compute_step_embeddings(c["src"], c["dst"], c["neg_dst"], c["times"], **kw)
        d1 = m.compute_node_temporal_embeddings(c["dst"], c["times"], **kw)
        one = m.compute_node_temporal_embeddings(c["dst"][5:6], c["times"][5:6], **kw)
        rev = m.compute_node_temporal_embeddings(c["dst"][::-1].copy(), c["times"][::-1].copy(), **kw)
    assert torch.equal(s, s3) and torch.equal(d, d3) and torch.equal(nd, n3) and torch.equal(d, d1)
    assert torch.equal(one[0], d[5]) and torch.equal(rev.flip(0), d)


def synthetic_setup(K, layers, dims=None, seed=3):
    """a bipartite graph with non-zero node features (row 0 included) and seeded parameters"""
    Fn, Ft = (172, 100) if dims is None else dims
    data, nf, ef = syn.make_bipartite_graph(60, 9, 6000, seed=seed, duplicate_time_every=5)
    rs = np.random.RandomState(seed + 1)
    nf = (0.5 * rs.standard_normal((nf.shape[0], Fn))).astype(np.float32)
    ef = np.ascontiguousarray(ef[:, :Fn]) if Fn <= ef.shape[1] else ef
    params = syn.make_graphmixer_params(seed + 2, K, num_layers=layers, node_feat_dim=Fn, edge_feat_dim=Fn, time_feat_dim=Ft)
    return data, nf, ef, params, Ft


def roots_of(data, n, seed):
    """n (node, time) roots: interactions' endpoints at their own times (histories of every length), plus node 1 before its first interaction"""
    rs = np.random.RandomState(seed)
    idx = rs.randint(0, data.num_interactions, n)
    nodes = np.where(rs.randint(0, 2, n) == 0, data.src_node_ids[idx], data.dst_node_ids[idx]).astype(np.int64)
    times = data.node_interact_times[idx].astype(np.float64)
    times[0] = data.node_interact_times.min() - 1.0               # precedes every interaction
    return nodes, times


def against_oracle(K, layers, G, n, dims=None, what=""):
    import torch
    data, nf, ef, params, Ft = synthetic_setup(K, layers, dims)
    m = make_model(nf, ef, data, params, K, layers, Ft)
    nodes, times = roots_of(data, n, 100 + n)
    with torch.no_grad():
        got = m.compute_node_temporal_embeddings(nodes, times, num_neighbors=K, time_gap=G)
    want = gmo.graphmixer_forward(params, nf, ef, adjacency(data), nodes, times, K, G, layers)
    parity.close(got.cpu().numpy(), want, f"graphmixer {what} K={K} L={layers} G={G} n={n}", "graphmixer embeddings vs restatement")
    return m, nodes, times, got


@pytest.mark.parametrize("K", [2, 10, 20, 32])
def test_token_counts(K):
    against_oracle(K, 2, 2000, 67)


@pytest.mark.parametrize("G", [1, 3, 2000, 5000])
def test_time_gaps(G):
    against_oracle(30, 2, G, 67)           # degrees reach ~1500 here: 5000 exceeds every one, 1 and 3 truncate almost all


@pytest.mark.parametrize("n", [1, 1537])
def test_root_counts(n):
    against_oracle(30, 2, 2000, n)          # 1537 is a multiple of no tile (16 roots, 64 token rows)


@pytest.mark.parametrize("dims,layers", [((16, 16), 1), ((32, 16), 3), ((16, 16), 3)])
def test_small_dims(dims, layers):
    against_oracle(4, layers, 2000, 45, dims=dims, what=f"dims={dims}")


def test_max_layers():
    from dyglib_amd import _capi
    against_oracle(10, _capi.DYGNN_MAX_LAYERS, 50, 21)


def test_non_default_stream_and_tensor_inputs():
    import torch
    m, nodes, times, want = against_oracle(20, 2, 2000, 130)
    st = torch.cuda.Stream(device=DEV)
    tn, tt = torch.from_numpy(nodes).to(DEV), torch.from_numpy(times).to(DEV)
    torch.cuda.synchronize()
    with torch.no_grad(), torch.cuda.stream(st):
        on_stream = m.compute_node_temporal_embeddings(nodes, times, num_neighbors=20, time_gap=2000)
        from_tensors = m.compute_node_temporal_embeddings(tn, tt, num_neighbors=20, time_gap=2000)
    st.synchronize()
    assert torch.equal(on_stream, want) and torch.equal(from_tensors, want)
    with torch.no_grad():
        a, b = m.compute_src_dst_node_temporal_embeddings(tn[:50], tn[50:100], tt[:50], num_neighbors=20, time_gap=2000)
        c, d = m.compute_src_dst_node_temporal_embeddings(nodes[:50], nodes[50:100], times[:50], num_neighbors=20, time_gap=2000)
    assert torch.equal(a, c) and torch.equal(b, d) and torch.equal(a, want[:50])


def test_empty_batch():
    import torch
    c, cfg, m = case_model("gen_k10_g7")
    with torch.no_grad():
        s, d = m.compute_src_dst_node_temporal_embeddings(c["src"][:0], c["dst"][:0], c["times"][:0], num_neighbors=10, time_gap=7)
    assert s.shape == d.shape == (0, 172)


def test_bad_arguments_and_unsupported_configs_raise_before_any_launch():
    import torch
    c, cfg, m = case_model("gen_k10_g7")
    a = (c["src"], c["dst"], c["times"])
    with torch.no_grad():
        with pytest.raises(AssertionError, match="greater than 0"):
            m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=0, time_gap=7)
        with pytest.raises(AssertionError, match="time_gap"):
            m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=10, time_gap=0)
        with pytest.raises(AssertionError, match="must equal num_tokens"):
            m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=20, time_gap=7)
        with pytest.raises(IndexError):
            m.compute_node_temporal_embeddings(np.array([10 ** 6]), np.array([1.0]), num_neighbors=10, time_gap=7)
    data, nf, ef, params, Ft = synthetic_setup(1, 1)
    from dyglib_amd import GraphMixer, get_neighbor_sampler
    one = GraphMixer(nf, ef, get_neighbor_sampler(data, "recent", seed=1, device=DEV), Ft, num_tokens=1, num_layers=1, device=DEV).to(DEV).eval()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="num_tokens 1 not supported"):
        one.compute_node_temporal_embeddings(np.array([1]), np.array([5.0]), num_neighbors=1, time_gap=7)
    wide = GraphMixer(np.zeros((nf.shape[0], 260), np.float32), ef, get_neighbor_sampler(data, "recent", seed=1, device=DEV), Ft, num_tokens=4,
                      num_layers=1, device=DEV).to(DEV).eval()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="feature dims > 256"):
        wide.compute_node_temporal_embeddings(np.array([1]), np.array([5.0]), num_neighbors=4, time_gap=7)


def test_autograd_recording_and_random_sampling_are_refused():
    import torch
    from dyglib_amd import get_neighbor_sampler
    c, cfg, m = case_model("gen_k10_g7")
    a = (c["src"], c["dst"], c["times"])
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=10, time_gap=7)
    m.train()
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.compute_step_embeddings(c["src"], c["dst"], c["neg_dst"], c["times"], num_neighbors=10, time_gap=7)
    with torch.no_grad():                                   # train mode without recording is the same forward (dropout is the training PR's)
        s, _ = m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=10, time_gap=7)
    parity.close(s.cpu().numpy(), gc.load_golden("graphmixer_gen_k10_g7")["src_emb"], "train mode, no_grad", "graphmixer embeddings vs reference")
    m.eval()
    m.set_neighbor_sampler(get_neighbor_sampler(c["data"], "uniform", seed=2, device=DEV))
    with torch.no_grad(), pytest.raises(NotImplementedError, match="recent"):
        m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=10, time_gap=7)
