"""The deferred pooled epilogue of the fused DyGFormer inference path (k_dygformer_fused3<.., PL = 3> + k_pooled_tail) against the
in-kernel epilogue (PL = 1).

Both forms run the same MFMA chains per output element and a column of an MFMA does not depend on its neighbours, so every embedding must
be equal BIT FOR BIT (torch.equal), whichever rows share a wave of the tail kernel.  DYGNN_POOLED_TAIL=1 / 0 puts a call on either form
whatever its size (unset, the size rule decides: the calls here are all below it).  Shapes: every kernel instance that has a deferred
form, a half-full last fused workgroup, a partial last tail workgroup (128 rows) and a 2-row last tile, the paired layout, groups with
their own padded lengths (the 1 / T_side scale), all-zero feature tables.  One case is also held to the oracle at the project's bar."""
import numpy as np
import pytest
import torch

from dyglib_amd import synthetic as syn
from oracle import dygformer_oracle as orc
from tests import golden_cases as gc
from tests import large_batch_cases as lb
from tests.parity import close_scaled
from tests.test_dygformer_gpu import build_model

pytestmark = pytest.mark.gpu


def both_forms(monkeypatch, call):
    """call() -> (src embeddings, dst embeddings) on the in-kernel form, then on the tail form; asserts equality, returns the tail's"""
    out = {}
    for form in ("0", "1"):
        monkeypatch.setenv("DYGNN_POOLED_TAIL", form)
        with torch.no_grad():
            out[form] = call()
    torch.cuda.synchronize()
    for k, t in zip(out["0"], out["1"]):
        assert torch.isfinite(k).all()
        assert torch.equal(k, t), float((k - t).abs().max())
    return out["1"]


@pytest.fixture(scope="module")
def full64():
    c = lb.build("full64")          # L = 64 / P = 2, 257 pairs, every late window full
    model, _ = build_model(c)
    model.impl = 3
    return c, model


def test_odd_batch_eight_wave_unpaired(full64, monkeypatch):
    """B = 257: 129 eight-wave workgroups, the last with one pair; 514 rows = 4 tail workgroups + 2 rows (a 2-row last tile)"""
    c, model = full64
    s, d = both_forms(monkeypatch, lambda: model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"]))
    assert s.shape == (257, 172) and d.shape == (257, 172)


def test_paired_layout(full64, monkeypatch):
    """[2, 130] with pos_neg_halves: workgroup w holds pairs w and w + 130, so column -> pair goes through pair_stride"""
    c, model = full64
    src, dst, t = c["src"][-130:], c["dst"][-130:], c["times"][-130:]
    neg = syn.random_negative_dst(np.random.RandomState(4), np.unique(c["data"].dst_node_ids), 130)
    args = (np.stack([src, src]), np.stack([dst, neg]), np.stack([t, t]))
    s, d = both_forms(monkeypatch, lambda: model.compute_src_dst_node_temporal_embeddings_many(*args, pos_neg_halves=True))
    with torch.no_grad():
        ns, nd = model.compute_src_dst_node_temporal_embeddings(src, neg, t)       # still on the tail form
    assert torch.equal(s[1], ns) and torch.equal(d[1], nd)


@pytest.mark.parametrize("B", [1, 9])
def test_four_wave_kernel(full64, monkeypatch, B):
    """calls of at most 256 pairs: one pair per four-wave workgroup; 2 and 18 rows"""
    c, model = full64
    both_forms(monkeypatch, lambda: model.compute_src_dst_node_temporal_embeddings(c["src"][-B:], c["dst"][-B:], c["times"][-B:]))


def test_128_token_pairs(monkeypatch):
    """L = 256 / P = 4: 128 tokens, one pair per eight-wave workgroup (k_dygformer_fused3<8, ., 8>), B = 5"""
    from dyglib_amd import DyGFormer, get_neighbor_sampler
    data, nf, ef = syn.make_bipartite_graph(40, 6, 9000, seed=23, duplicate_time_every=5)
    params = syn.make_dygformer_params(9, patch_size=4)
    model = DyGFormer(nf, ef, get_neighbor_sampler(data, "recent", seed=1, device="cuda:0"), 100, 50, patch_size=4, num_layers=2, num_heads=2,
                      dropout=0.1, max_input_sequence_length=256, device="cuda:0")
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    model = model.to("cuda:0").eval()
    src, dst, t = data.src_node_ids[-5:], data.dst_node_ids[-5:], data.node_interact_times[-5:]
    taps = {}
    with torch.no_grad():
        model.compute_src_dst_node_temporal_embeddings(src, dst, t, _taps=taps)
    assert sum(taps["seq_lens"].cpu().tolist()) // 4 > 64          # more than 64 tokens: the one-pair shape
    both_forms(monkeypatch, lambda: model.compute_src_dst_node_temporal_embeddings(src, dst, t))


def test_groups_with_their_own_padded_lengths_and_the_oracle(monkeypatch):
    """three calls of 40 pairs of the hub graph (P = 4, L = 48) in one launch: every group scales its sums by its own 1 / T_side.  Also
    against the oracle, call by call, at 1e-4 * max(1, max|ref|)."""
    c = gc.build_case("hub_p4_l48")
    model, _ = build_model(c)
    model.impl = 3
    d = c["data"]
    rows = [np.arange(0, 40), np.arange(100, 140), np.arange(260, 300)]
    src, dst, t = (np.stack([arr[r] for r in rows]) for arr in (d.src_node_ids, d.dst_node_ids, d.node_interact_times))
    s, de = both_forms(monkeypatch, lambda: model.compute_src_dst_node_temporal_embeddings_many(src, dst, t))
    adj = orc.OracleAdjacency(d.src_node_ids, d.dst_node_ids, d.edge_ids, d.node_interact_times)
    lens = []
    for i in range(3):
        taps = {}
        with torch.no_grad():
            model.compute_src_dst_node_temporal_embeddings(src[i], dst[i], t[i], _taps=taps)
            os_, od = orc.dygformer_forward(c["params"], c["node_feat"], c["edge_feat"], adj, src[i], dst[i], t[i], 4, 48)
        lens.append(tuple(taps["seq_lens"].cpu().tolist()))
        close_scaled(s[i].cpu().numpy(), os_.numpy(), f"pooled tail, call {i} src emb")
        close_scaled(de[i].cpu().numpy(), od.numpy(), f"pooled tail, call {i} dst emb")
    assert len(set(lens)) == 3, lens          # the groups really were padded to different lengths


def test_all_zero_feature_tables(monkeypatch):
    """node and edge table all zero (table_flags 3: both channels leave the projection walk)"""
    from dyglib_amd import DyGFormer, get_neighbor_sampler
    data, nf, ef = syn.make_bipartite_graph(600, 80, 20000, seed=21, edge_feat_kind="zeros")
    assert not nf.any() and not ef.any()
    params = syn.make_dygformer_params(7, patch_size=2)
    model = DyGFormer(nf, ef, get_neighbor_sampler(data, "recent", seed=1, device="cuda:0"), 100, 50, patch_size=2, num_layers=2, num_heads=2,
                      dropout=0.1, max_input_sequence_length=64, device="cuda:0")
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    model = model.to("cuda:0").eval()
    assert model.table_flags == 3
    src, dst, t = data.src_node_ids[-259:], data.dst_node_ids[-259:], data.node_interact_times[-259:]
    both_forms(monkeypatch, lambda: model.compute_src_dst_node_temporal_embeddings(src, dst, t))
