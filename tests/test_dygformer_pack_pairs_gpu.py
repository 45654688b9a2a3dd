"""Token compaction and pair packing of the fused DyGFormer inference kernels on the GPU.

Every inference kernel computes a pair's distinct tokens once (real source tokens, real destination tokens, ONE padding token); large
untapped launches lay pairs of 1 .. 4 token tiles eight tiles to a workgroup (DYGNN_PACK_PAIRS = 1 / 0 puts any / no eligible call on
that kernel).  Rows are built with prescribed history lengths — the query time lies between a node's k-th and (k + 1)-th interaction —
so that the compact token count sits on every tile boundary.  Each case is held to the oracle (1e-4 * max(1, |ref|), the observed
error is printed) and the packed kernel to the unpacked one bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from dyglib_amd import _capi
from dyglib_amd import synthetic as syn
from oracle import dygformer_oracle as orc
from tests import golden_cases as gc
from tests.parity import close, close_scaled
from tests.test_dygformer_gpu import build_model

gpu = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _graph():
    data, nf, ef = syn.make_bipartite_graph(300, 40, 6000, seed=41)
    adj = orc.OracleAdjacency(data.src_node_ids, data.dst_node_ids, data.edge_ids, data.node_interact_times)
    ev_node = np.concatenate([data.src_node_ids, data.dst_node_ids])
    ev_time = np.concatenate([data.node_interact_times, data.node_interact_times])
    tu = np.unique(data.node_interact_times)
    cand = np.concatenate([(tu[1:] + tu[:-1]) / 2, [tu[-1] + 1.0]])         # query times that tie with no interaction
    return data, nf, ef, adj, ev_node, ev_time, cand


@functools.lru_cache(maxsize=None)
def _model(P, L):
    from dyglib_amd import DyGFormer, get_neighbor_sampler
    data, nf, ef = _graph()[:3]
    params = syn.make_dygformer_params(52, patch_size=P, num_layers=2)
    sampler = get_neighbor_sampler(data, "recent", seed=1, device="cuda:0")
    model = DyGFormer(nf, ef, sampler, 100, 50, patch_size=P, num_layers=2, num_heads=2, dropout=0.1, max_input_sequence_length=L, device="cuda:0")
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    model = model.to("cuda:0").eval()
    model.impl = 3
    return model, params


def _rows(P, L, wanted):
    """(src, dst, t) rows whose real-token counts are the wanted (R_s, R_d): R = ceil((min(len, L - 1) + 1) / P), len = the node's
    interactions before t.  Deterministic: the first query time and the first two distinct nodes that fit."""
    _, _, _, _, ev_node, ev_time, cand = _graph()
    n_nodes = int(ev_node.max()) + 1
    step = max(1, cand.size // 400)
    tables = []
    for t in cand[::step].tolist() + [float(cand[-1])]:
        ln = np.bincount(ev_node[ev_time < t], minlength=n_nodes)
        R = -(-(np.minimum(ln, L - 1) + 1) // P)
        R[0] = -1                                                           # node 0 is the padding node
        tables.append((t, R))
    src, dst, tt = [], [], []
    for k, (rs_, rd_) in enumerate(wanted):
        for t, R in tables[k % 7:] + tables[:k % 7]:                      # different rows start at different times: not all at one t
            us, vs = np.flatnonzero(R == rs_), np.flatnonzero(R == rd_)
            hit = [(u, v) for u in us[:3] for v in vs[:3] if u != v]
            if hit:
                src.append(hit[0][0]); dst.append(hit[0][1]); tt.append(t)
                break
        else:
            raise AssertionError(f"no row with (R_s, R_d) = {(rs_, rd_)} in the test graph")
    return np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64), np.array(tt, dtype=np.float64)


def _compact_tokens(P, L, wanted):
    T_s, T_d = max(w[0] for w in wanted), max(w[1] for w in wanted)
    return [rs_ + rd_ + ((T_s - rs_) + (T_d - rd_) > 0) for rs_, rd_ in wanted]


def _forms(monkeypatch, fn):
    """fn() on the packed kernel and on the unpacked deferred-tail kernel"""
    out = {}
    for pack in ("1", "0"):
        monkeypatch.setenv("DYGNN_PACK_PAIRS", pack)
        monkeypatch.setenv("DYGNN_POOLED_TAIL", "1")
        with torch.no_grad():
            out[pack] = fn()
    monkeypatch.delenv("DYGNN_PACK_PAIRS")
    monkeypatch.delenv("DYGNN_POOLED_TAIL")
    return out["1"], out["0"]


def _check(monkeypatch, P, L, wanted, what):
    model, params = _model(P, L)
    _, nf, ef, adj = _graph()[:4]
    src, dst, t = _rows(P, L, wanted)
    with torch.no_grad():
        os_, od = orc.dygformer_forward(params, nf, ef, adj, src, dst, t, P, L)
    (ps, pd), (us, ud) = _forms(monkeypatch, lambda: model.compute_src_dst_node_temporal_embeddings(src, dst, t))
    with torch.no_grad():
        ds_, dd = model.compute_src_dst_node_temporal_embeddings(src, dst, t)             # the default form of a call of this size
    e = max(close_scaled(ps.cpu().numpy(), os_.numpy(), f"{what}: packed src emb"), close_scaled(pd.cpu().numpy(), od.numpy(), f"{what}: packed dst emb"))
    print(f"{what}: {len(wanted)} pairs, compact tokens {_compact_tokens(P, L, wanted)}, max |err| vs the oracle {e:.3e} (max |ref| {float(os_.abs().max()):.3g})")
    assert torch.equal(ps, us) and torch.equal(pd, ud), what
    assert torch.equal(ps, ds_) and torch.equal(pd, dd), what


# (R_s, R_d) of a call at L = 64, P = 2 that pads to 32 + 32 tokens (its longest row has no padding at all).  Compact tokens
# 3, 16, 17, 32, 33, 48, 49, 64 (with and without a padding token), then ten pairs of one tile: eight of them fill a workgroup
BOUNDARY = [(1, 1), (7, 8), (8, 8), (15, 16), (16, 16), (23, 24), (24, 24), (32, 32), (31, 32), (32, 31), (16, 32), (32, 1),
            (1, 2), (2, 3), (1, 5), (3, 3), (4, 2), (6, 5), (2, 2), (5, 1), (7, 7), (1, 14)]


@gpu
def test_token_counts_on_every_tile_boundary(monkeypatch):
    tc = _compact_tokens(2, 64, BOUNDARY)
    assert {3, 16, 17, 32, 33, 48, 49, 64} <= set(tc)
    tiles = np.array([-(-x // 16) for x in tc], dtype=np.int32)
    wg, fw = np.empty_like(tiles), np.empty_like(tiles)
    used = _capi.load().dygnn_dygformer_pack_plan_host(tiles.ctypes.data, tiles.size, wg.ctypes.data, fw.ctypes.data)
    assert used <= (tiles.size + 1) // 2 and np.bincount(wg).max() == 8           # eight one-tile pairs share a workgroup
    _check(monkeypatch, 2, 64, BOUNDARY, "tile boundaries")


@gpu
def test_call_padded_shorter_than_L_with_an_odd_source_side(monkeypatch):
    # T_s = 5, T_d = 7: one tile holds source tokens, destination tokens and the padding token
    _check(monkeypatch, 2, 64, [(5, 3), (2, 7), (1, 1), (5, 7), (3, 2), (4, 6), (5, 1)], "T_s = 5, T_d = 7")


@gpu
@pytest.mark.parametrize("P,L,wanted", [
    (1, 32, [(32, 32), (1, 1), (7, 8), (8, 8), (16, 15), (17, 20), (30, 32), (2, 31), (9, 3)]),
    (4, 48, [(12, 12), (1, 1), (3, 12), (12, 2), (7, 8), (8, 8), (5, 11), (2, 2), (11, 12)]),
])
def test_patch_sizes(monkeypatch, P, L, wanted):
    _check(monkeypatch, P, L, wanted, f"P = {P}, L = {L}")


@gpu
@pytest.mark.parametrize("wanted", [[(9, 30)], [(32, 32)], [(32, 32), (3, 2), (17, 16), (1, 1), (20, 28), (8, 7), (12, 12)]], ids=["B1", "B1_full", "B7"])
def test_one_pair_and_odd_batches(monkeypatch, wanted):
    _check(monkeypatch, 2, 64, wanted, f"B = {len(wanted)}")


@gpu
@pytest.mark.parametrize("pos_neg", [False, True])
def test_independently_padded_groups_in_one_launch(monkeypatch, pos_neg):
    """Four calls of one launch, each padded on its own (32 + 32, 5 + 7, 20 + 9 and 32 + 12 tokens); with pos_neg_halves calls 2 and 3 are the
    negative calls of calls 0 and 1 (same sources and times).  The packed launch against the separate unpacked calls."""
    model, _ = _model(2, 64)
    a = _rows(2, 64, BOUNDARY[:12])
    b = _rows(2, 64, [(5, 3), (2, 7), (1, 1), (5, 7), (3, 2), (4, 6), (5, 1), (2, 2), (1, 4), (3, 3), (4, 4), (5, 5)])
    if pos_neg:
        rs = np.random.RandomState(3)
        groups = [a, b, (a[0], rs.randint(1, 340, a[1].size), a[2]), (b[0], rs.randint(1, 340, b[1].size), b[2])]
    else:
        groups = [a, b, _rows(2, 64, [(20, 9), (1, 1), (7, 8), (20, 1), (3, 9), (16, 1), (2, 2), (8, 8), (10, 6), (4, 4), (1, 9), (19, 9)]),
                  _rows(2, 64, [(32, 12), (1, 1), (20, 12), (32, 1), (4, 12), (16, 12), (5, 5), (31, 2), (24, 8), (8, 8), (30, 12), (6, 6)])]
    src, dst, t = (np.stack([g[i] for g in groups]) for i in range(3))
    monkeypatch.setenv("DYGNN_PACK_PAIRS", "1")
    with torch.no_grad():
        ms, md = model.compute_src_dst_node_temporal_embeddings_many(src, dst, t, pos_neg_halves=pos_neg)
    monkeypatch.setenv("DYGNN_PACK_PAIRS", "0")
    with torch.no_grad():
        for i in range(4):
            s1, d1 = model.compute_src_dst_node_temporal_embeddings(src[i], dst[i], t[i])
            assert torch.equal(ms[i], s1) and torch.equal(md[i], d1), (pos_neg, i)


@gpu
def test_tapped_call_with_padding(monkeypatch):
    """Taps keep the padded [B][T_max] layout: the padding token's row is written to every padding row.  Encoder input and both layers
    against the oracle, padding rows included; the embeddings are those of the untapped call, packed or not, bit for bit."""
    P, L = 2, 64
    wanted = BOUNDARY[:14]
    model, params = _model(P, L)
    _, nf, ef, adj = _graph()[:4]
    src, dst, t = _rows(P, L, wanted)
    otaps, taps = {}, {}
    with torch.no_grad():
        orc.dygformer_forward(params, nf, ef, adj, src, dst, t, P, L, taps=otaps)
        ts, td = model.compute_src_dst_node_temporal_embeddings(src, dst, t, _taps=taps)
    T = otaps["encoder_input"].shape[1]
    assert T == 64 and min(_compact_tokens(P, L, wanted)) == 3            # rows with 61 padding rows among them
    close_scaled(taps["encoder_input"][:, :T].cpu().numpy(), otaps["encoder_input"].numpy(), "tapped encoder input, padding rows included")
    for l in range(2):
        close_scaled(taps["layer_outputs"][l][:, :T].cpu().numpy(), otaps["layer_outputs"][l].numpy(), f"tapped layer {l}, padding rows included (internal tap, scaled bar)")
    (ps, pd), (us, ud) = _forms(monkeypatch, lambda: model.compute_src_dst_node_temporal_embeddings(src, dst, t))
    assert torch.equal(ts, ps) and torch.equal(td, pd) and torch.equal(ts, us) and torch.equal(td, ud)


@gpu
def test_128_token_fixture_still_passes(monkeypatch):
    """L = 512 / P = 8: one pair per workgroup, nothing to pack (compaction only) — DYGNN_PACK_PAIRS = 1 leaves the call where it was."""
    c = gc.build_case("bip_p8_l512")
    g = gc.load_golden("bip_p8_l512")
    model, _ = build_model(c)
    model.impl = 3
    (ps, pd), (us, ud) = _forms(monkeypatch, lambda: model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"]))
    close(ps.cpu().numpy(), g["src_emb"], "bip_p8_l512 compacted src emb")
    close(pd.cpu().numpy(), g["dst_emb"], "bip_p8_l512 compacted dst emb")
    assert torch.equal(ps, us) and torch.equal(pd, ud)


@gpu
def test_one_group_per_pair_is_not_packed_and_keeps_its_bits(monkeypatch):
    """The plan lives in the CallDims slots that the groups of a call leave free; with one group per pair there are none, and the launch
    stays unpacked whatever DYGNN_PACK_PAIRS says.  Every pair is its own call here: no padding beyond its own windows."""
    model, _ = _model(2, 64)
    src, dst, t = _rows(2, 64, BOUNDARY[:9])
    (ps, pd), (us, ud) = _forms(monkeypatch, lambda: model.compute_src_dst_node_temporal_embeddings(src, dst, t, _group_size=1))
    assert torch.equal(ps, us) and torch.equal(pd, ud)
    with torch.no_grad():
        for i in range(3):
            s1, d1 = model.compute_src_dst_node_temporal_embeddings(src[i:i + 1], dst[i:i + 1], t[i:i + 1])
            assert torch.equal(ps[i:i + 1], s1) and torch.equal(pd[i:i + 1], d1), i
