"""The host copy of the training path's dropout generator (oracle/dropout.py, restating dyglib_amd/csrc/dropout.h) and the TGAT oracle's
train-mode numbering (oracle/tgat_oracle.py: TrainDropout), on CPU.  tests/test_tgat_configs_gpu.py compares the HIP training path with
the masked oracle."""
import numpy as np
import pytest
import torch

from dyglib_amd import synthetic as syn
from oracle import dropout as drp
from oracle import dygformer_oracle as orc
from oracle import tgat_oracle as torc

M32 = 0xFFFFFFFF


def _mix32_int(x):          # dropout.h mix32 in plain Python integers: an independent check of the uint64-masked numpy version
    x &= M32
    x ^= x >> 16; x = (x * 0x7FEB352D) & M32; x ^= x >> 15; x = (x * 0x846CA68B) & M32; x ^= x >> 16
    return x


def test_mix32_matches_integer_arithmetic():
    xs = [0, 1, 2, 0x7FFFFFFF, 0x80000000, M32, 0x9E3779B9, 123456789]
    xs += np.random.RandomState(0).randint(0, 2 ** 32, size=200, dtype=np.uint64).tolist()
    got = drp.mix32(np.array(xs, dtype=np.uint64))
    assert got.dtype == np.uint32
    assert got.tolist() == [_mix32_int(x) for x in xs]


def test_make_drop_keys_threshold_and_scale():
    seed = (0x1234ABCD << 32) | 0x89ABCDEF
    d = drp.make_drop(0.1, seed)
    assert d.key0 == 0x89ABCDEF
    assert d.key1 == (0x1234ABCD * 0x85EBCA6B + 0x165667B1) & M32
    p32 = float(np.float32(0.1))                                   # the ABI takes a float: 0.1 arrives as 0.100000001490116...
    assert d.thresh == int(p32 * 2.0 ** 32) and d.thresh != int(0.1 * 2.0 ** 32)
    for p in (0.1, 0.2, 0.5, 0.9):
        assert drp.make_drop(p, 3).scale == np.float32(1.0 / (1.0 - float(np.float32(p))))
        assert drp.make_drop(p, 3).scale.dtype == np.float32
    assert drp.make_drop(0.1, 7).site_key(3) == _mix32_int(7 + 0x9E3779B9 * 4) ^ ((0 * 0x85EBCA6B + 0x165667B1) & M32)


def test_p0_keeps_everything_at_scale_1():
    m = drp.mask(0.0, 99, 5, np.arange(100000, dtype=np.int64))
    assert m.dtype == np.float32 and (m == 1.0).all()


def test_keep_fraction_within_binomial_bounds():
    n, p = 1 << 20, 0.1
    for site in (0, 1, 7):
        m = drp.mask(p, 1234567, site, np.arange(n, dtype=np.int64))
        kept = int((m != 0).sum())
        sd = np.sqrt(n * p * (1 - p))
        assert abs(kept - n * (1 - p)) < 6 * sd, (site, kept)
        assert set(np.unique(m).tolist()) == {0.0, float(np.float32(1 / (1 - np.float32(p))))}


def test_sites_and_seeds_draw_different_masks():
    idx = np.arange(4096, dtype=np.int64)
    a = drp.mask(0.5, 11, 0, idx)
    assert not np.array_equal(a, drp.mask(0.5, 11, 1, idx))
    assert not np.array_equal(a, drp.mask(0.5, 12, 0, idx))
    assert not np.array_equal(a, drp.mask(0.5, 11 + (1 << 32), 0, idx))          # the seed's high word reaches the mask (key1)


def test_index_fold():
    lo = np.array([0, 1, 12345, M32 - 1, M32], dtype=np.int64)
    assert drp.fold_index(lo).tolist() == lo.tolist()                                    # identity below 2^32
    hi = np.array([1 << 32, (1 << 32) + 5, (3 << 32) + 7, (1 << 40) + M32], dtype=np.uint64)
    want = [((int(i) & M32) + 0x27D4EB2F * (int(i) >> 32)) & M32 for i in hi]
    assert drp.fold_index(hi).tolist() == want
    d = drp.make_drop(0.3, 5)
    assert np.array_equal(d.mask(2, hi), d.mask(2, np.array(want, dtype=np.int64)))     # mask(idx) draws at the folded index


def _graph(L):
    data, nf, ef = syn.make_bipartite_graph(30, 8, 400, seed=3, edge_feat_dim=8)
    nf = np.random.RandomState(4).standard_normal((nf.shape[0], 8)).astype(np.float32)
    params = syn.make_tgat_params(5, node_feat_dim=8, edge_feat_dim=8, time_feat_dim=8, num_layers=L)
    adj = orc.OracleAdjacency(data.src_node_ids, data.dst_node_ids, data.edge_ids, data.node_interact_times)
    E = data.num_interactions
    ids = np.concatenate([data.src_node_ids[E - 6:], data.dst_node_ids[E - 6:]])
    t = np.concatenate([data.node_interact_times[E - 6:]] * 2)
    return params, torch.from_numpy(nf), torch.from_numpy(ef), adj, ids, t


@pytest.mark.parametrize("L,k", [(1, 4), (2, 3), (3, 2)])
def test_oracle_visits_every_training_row_once(L, k):
    """per computed level l, the rows the oracle's calls cover are exactly 0 .. n[l]-1, each once (tgat_train.hip's layout)"""
    params, nf, ef, adj, ids, t = _graph(L)
    dr = torc.TrainDropout(0.1, 17)
    torc.node_embeddings(params, nf, ef, adj, ids, t, L, k, 2, dropout=dr)
    n = len(ids)
    for l in range(L, 0, -1):
        rows = np.concatenate([np.arange(r0, r0 + c) for r0, c in dr.visits[l]])
        assert len(rows) == n and np.array_equal(np.sort(rows), np.arange(n)), l
        n *= 1 + k
    assert dr.n[0] == n


def test_oracle_dropout_p0_is_the_plain_oracle_and_p01_is_not():
    params, nf, ef, adj, ids, t = _graph(2)
    plain = torc.node_embeddings(params, nf, ef, adj, ids, t, 2, 3, 2)
    assert torch.equal(torc.node_embeddings(params, nf, ef, adj, ids, t, 2, 3, 2, dropout=torc.TrainDropout(0.0, 17)), plain)
    a = torc.node_embeddings(params, nf, ef, adj, ids, t, 2, 3, 2, dropout=torc.TrainDropout(0.1, 17))
    b = torc.node_embeddings(params, nf, ef, adj, ids, t, 2, 3, 2, dropout=torc.TrainDropout(0.1, 18))
    assert torch.isfinite(a).all() and not torch.equal(a, plain) and not torch.equal(a, b)
