"""The pooled layer's per-side token sums on the GPU (csrc/fused3_device.h: row_sums8): sums of gelu(h) and of the residual over
a tile's tokens by a reduce-scatter, stored one word per (row, side).

Rows with prescribed history lengths (tests/test_dygformer_pack_pairs_gpu.py) put the compact token order where the sums change form.  One call
of 13 pairs at L = 64 / P = 2, padded to 32 + 32 tokens; (R_s, R_d) real tokens per side, m = 32 - R padding tokens per side, compact order =
source tokens, destination tokens, ONE padding token:

* (5, 6): 12 tokens — source, destination and the padding token (m_s = 27, m_d = 26, both weights in front of the sum) in one tile;
* (1, 20), (17, 9): the source side ends at column 1 of a tile; (15, 20), (31, 20): at column 15;
* (7, 9), (20, 12): R_s + R_d = 16, 32 — the padding token alone in its tile (a straddling tile with fifteen +0 lanes);
* (10, 32): m_s > 0, m_d = 0; (32, 10): the mirror — the padding token counts on one side only;
* (32, 32): 64 tokens, no padding token, the sides meet on a tile edge: every tile is a one-side tile;
* (16, 16), (1, 1), (32, 31): a side boundary on a tile edge with the padding token behind it, the shortest pair, 64 tokens with a padding token.

and the L = 512 / P = 8 fixture of the reference, for the 128-token instance.

Every form is held to the oracle at the embeddings' bar (tests/parity.close: 1e-4 absolute, as tests/test_dygformer_pooled_ffn_gpu.py holds the
same quantity; the observed maximum is printed), and the forms to each other bit for bit: the four-wave kernel (a small call), the eight-wave
kernel (257 pairs, the same rows over and over: DYGNN_SMALL_BATCH_KERNELS is read once per process), the packed kernel with the deferred
tail, and the same rows as one of the calls of a compute_src_dst_node_temporal_embeddings_many launch.

Not built here: one pair's row computed once in a one-side tile and once in a straddling tile.  A side always holds its target node, so no
side has zero real tokens, and an embedding depends on every token of its pair through the attention: moving a row's tokens to another
column changes the pair and with it the row.  The two forms are one routine fed +0 in the lanes that do not count;
tests/test_dygformer_pool_sums_cpu.py holds their bits equal on the simulated lanes, and the (32, 32) pair (one-side tiles only) and the
straddling pairs above are held to the oracle here."""
import functools

import numpy as np
import pytest
import torch

from oracle import dygformer_oracle as orc
from tests import golden_cases as gc
from tests.parity import close
from tests.test_dygformer_gpu import build_model
from tests.test_dygformer_pack_pairs_gpu import _compact_tokens, _graph, _model, _rows

gpu = pytest.mark.gpu

P, L = 2, 64
WANTED = [(5, 6), (1, 20), (17, 9), (15, 20), (31, 20), (7, 9), (20, 12), (10, 32), (32, 10), (32, 32), (16, 16), (1, 1), (32, 31)]


def test_the_rows_are_the_cases_they_are_meant_to_be():
    assert len(WANTED) <= 16
    T_s, T_d = max(w[0] for w in WANTED), max(w[1] for w in WANTED)
    assert (T_s, T_d) == (32, 32)
    tc = dict(zip(WANTED, _compact_tokens(P, L, WANTED)))
    pad = lambda w: tc[w] - 1 if tc[w] > w[0] + w[1] else None      # the padding token, or none
    assert tc[(5, 6)] == 12 and pad((5, 6)) == 11                   # one tile: source, destination, padding
    assert {w[0] % 16 for w in WANTED} >= {1, 15}                   # the source side ends inside a tile at columns 1 and 15
    assert (17, 9) in tc and (31, 20) in tc                         # ... also in the second tile
    assert pad((7, 9)) == 16 and pad((20, 12)) == 32                # the padding token alone in its tile
    assert tc[(10, 32)] == 43 and tc[(32, 10)] == 43                # m_s > 0, m_d = 0 and the mirror
    assert tc[(32, 32)] == 64 and pad((32, 32)) is None
    assert len(_rows(P, L, WANTED)[0]) == len(WANTED)               # the test graph has such rows


@functools.lru_cache(maxsize=None)
def _case():
    _, nf, ef, adj = _graph()[:4]
    src, dst, t = _rows(P, L, WANTED)
    with torch.no_grad():
        os_, od = orc.dygformer_forward(_model(P, L)[1], nf, ef, adj, src, dst, t, P, L)
    return src, dst, t, os_.numpy(), od.numpy()


def _held(what, s, d, os_, od):
    e = max(close(s.cpu().numpy(), os_, f"pool sums {what}: src emb"), close(d.cpu().numpy(), od, f"pool sums {what}: dst emb"))
    print(f"pool sums, {what}: max |emb - oracle| {e:.3e} (max |ref| {max(np.abs(os_).max(), np.abs(od).max()):.3g})")


@gpu
def test_every_form_against_the_oracle_and_bit_for_bit_against_each_other(monkeypatch):
    model = _model(P, L)[0]
    src, dst, t, os_, od = _case()
    B = len(src)
    with torch.no_grad():
        s4, d4 = model.compute_src_dst_node_temporal_embeddings(src, dst, t)              # a small call: four-wave workgroups, one pair each
    _held("four-wave kernel", s4, d4, os_, od)
    rep = np.arange(257) % B
    with torch.no_grad():
        s8, d8 = model.compute_src_dst_node_temporal_embeddings(src[rep], dst[rep], t[rep])      # eight-wave workgroups, two pairs each
    _held("eight-wave kernel", s8[:B], d8[:B], os_, od)
    monkeypatch.setenv("DYGNN_PACK_PAIRS", "1")
    monkeypatch.setenv("DYGNN_POOLED_TAIL", "1")
    with torch.no_grad():
        sp, dp = model.compute_src_dst_node_temporal_embeddings(src, dst, t)              # packed, deferred tail
        # four calls of one launch, each padded on its own: the rows, the rows reversed (other slots, other partners), and two halves
        groups = [np.arange(B), np.arange(B)[::-1].copy(), np.arange(B) % 6, 6 + np.arange(B) % 7]
        ms, md = model.compute_src_dst_node_temporal_embeddings_many(np.stack([src[g] for g in groups]), np.stack([dst[g] for g in groups]),
                                                                     np.stack([t[g] for g in groups]))
    monkeypatch.delenv("DYGNN_PACK_PAIRS")
    monkeypatch.delenv("DYGNN_POOLED_TAIL")
    _held("packed kernel, deferred tail", sp, dp, os_, od)
    _held("a call of a many-call launch", ms[0], md[0], os_, od)
    assert torch.equal(s8, s4[rep]) and torch.equal(d8, d4[rep])
    assert torch.equal(sp, s4) and torch.equal(dp, d4)
    assert torch.equal(ms[0], s4) and torch.equal(md[0], d4)
    assert torch.equal(ms[1], s4.flip(0)) and torch.equal(md[1], d4.flip(0))
    with torch.no_grad():
        # call 2 pads to 31 + 20 tokens, not 32 + 32 (other multiplicities of the padding token): the single calls of the same rows are the reference
        for i in (2, 3):
            g = groups[i]
            s1, d1 = model.compute_src_dst_node_temporal_embeddings(src[g], dst[g], t[g])
            assert torch.equal(ms[i], s1) and torch.equal(md[i], d1), i


@gpu
def test_the_128_token_instance_on_the_reference_fixture(monkeypatch):
    c = gc.build_case("bip_p8_l512")
    g = gc.load_golden("bip_p8_l512")
    model, _ = build_model(c)
    model.impl = 3
    with torch.no_grad():
        s, d = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"])
        ts, td = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], _taps={})      # PL = 2: the same sums
    monkeypatch.setenv("DYGNN_POOLED_TAIL", "1")
    with torch.no_grad():
        s3, d3 = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"])                # PL = 3 and k_pooled_tail
    monkeypatch.delenv("DYGNN_POOLED_TAIL")
    e = max(close(s.cpu().numpy(), g["src_emb"], "pool sums bip_p8_l512: src emb"), close(d.cpu().numpy(), g["dst_emb"], "pool sums bip_p8_l512: dst emb"))
    print(f"pool sums, 128-token kernel: max |emb - fixture| {e:.3e}")
    assert torch.equal(s, ts) and torch.equal(d, td) and torch.equal(s, s3) and torch.equal(d, d3)
