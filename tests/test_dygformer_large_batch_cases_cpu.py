"""The recipes of tests/large_batch_cases.py have the properties their GPU tests rely on — established with the oracle alone, no GPU:
padded lengths, tokens per pair, dense row counts and their remainders, odd batch sizes, and that every size lies ABOVE the library's
small-call thresholds (read from fused3_host.h: a later change of kSmallBatchPairs fails here instead of silently turning the
eight-wave tests into four-wave ones)."""
import os
import re

import numpy as np
import pytest

from oracle import dygformer_oracle as orc
from tests import large_batch_cases as lb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FFN_ROWS_PER_WG = 128          # k_ffn_bwd<8>: 8 waves of 16 dense token rows
MAX_TOKENS_TWO_PAIRS = 64      # two pairs share an eight-wave workgroup up to this many tokens per pair


def _small_batch_pairs() -> int:
    with open(os.path.join(ROOT, "dyglib_amd", "csrc", "fused3_host.h")) as f:
        m = re.findall(r"constexpr\s+int64_t\s+kSmallBatchPairs\s*=\s*(\d+)\s*;", f.read())
    assert len(m) == 1, m
    return int(m[0])


def _padded_lengths(data, src, dst, times, P, L):
    adj = orc.OracleAdjacency(data.src_node_ids, data.dst_node_ids, data.edge_ids, data.node_interact_times)
    s_id, _, _ = orc.first_hop_windows(adj, src, times, P, L)
    d_id, _, _ = orc.first_hop_windows(adj, dst, times, P, L)
    return (s_id.shape[1], d_id.shape[1]), s_id, d_id


def _shape(name, *args):
    fn, P, L, want = lb.RECIPES[name]
    data, nf, ef, params, (src, dst, times) = fn(*args)
    assert src.shape == dst.shape == times.shape and src.dtype == np.int64 and times.dtype == np.float64
    lens, s_id, d_id = _padded_lengths(data, src, dst, times, P, L)
    assert [lens] == want, (name, lens)
    B, T = len(src), (lens[0] + lens[1]) // P
    return B, T, B * T, data, nf, (s_id, d_id)


def test_thresholds_lie_below_every_recipe():
    k = _small_batch_pairs()
    assert k == 256                                   # the figures in the recipes' docstrings assume it
    sizes = {name: _shape(name, *a)[:3] for name, a in (("full64", ()), ("full64", (401,)), ("ragged40", ()), ("hub14", ()))}
    for name, (B, T, M) in sizes.items():
        assert B > k and B % 2 == 1, (name, B)        # eight-wave kernels, last workgroup half empty
        assert T <= MAX_TOKENS_TWO_PAIRS, (name, T)   # two pairs per workgroup
    assert 3 * 87 > k and 87 <= k                     # hub_groups: the launch is large, every call alone is small
    assert 200 <= k < 400                             # one pass of two 200-pair calls against two separate calls
    for name in ("full64", "ragged40"):
        assert sizes[name][2] > 64 * k, name          # k_ffn_bwd<8>
    assert _shape("hub14")[2] <= 64 * k               # k_ffn_bwd<4> after the eight-wave forward: the mixed combination


@pytest.mark.parametrize("B", [257, 401])
def test_full64(B):
    got_B, T, M, data, nf, (s_id, d_id) = _shape("full64", B)
    assert (got_B, T, M) == (B, 64, 64 * B)
    if B == 257:
        assert M == 16448 and M % FFN_ROWS_PER_WG == 64          # the last workgroup of k_ffn_bwd<8>: waves 0-3 full, 4-7 idle
    assert (s_id[:3, 1:] == 0).all() and (d_id[:3, 1:] == 0).all()          # the first interactions: empty histories
    assert (s_id[3:] != 0).sum(1).max() == 64 and (d_id[3:] != 0).sum(1).max() == 64
    assert not nf[0].any() and nf[1:].any(1).all()               # padding row zero, every other node featured


def test_ragged40():
    B, T, M, data, nf, (s_id, d_id) = _shape("ragged40")
    assert (B, T, M) == (411, 40, 16440)
    T_src = lb.RECIPES["ragged40"][3][0][0] // lb.RECIPES["ragged40"][1]
    assert T % 16 == 8 and T_src == 20 and T_src % 16 != 0       # the last tile is half empty; tile 1 holds tokens of both sides
    rem = M % FFN_ROWS_PER_WG
    assert rem == 56 and divmod(rem, 16) == (3, 8)               # waves 0-2 full, wave 3 has 8 valid rows, waves 4-7 none
    assert (s_id[:3, 1:] == 0).all() and (d_id[:3, 1:] == 0).all()
    assert not nf[0].any() and nf[1:].any(1).all()


def test_hub14():
    B, T, M, data, nf, _ = _shape("hub14")
    assert (B, T, M) == (257, 14, 3598)
    assert T % 4 != 0 and T < 16                                 # k_attn_bwd's scalar path, one partly filled tile per pair
    assert lb.RECIPES["hub14"][3][0][0] != lb.RECIPES["hub14"][3][0][1]          # S_src != S_dst


def test_hub_groups():
    fn, P, L, want = lb.RECIPES["hub_groups"]
    data, nf, ef, params, (src, dst, times) = fn()
    assert src.shape == dst.shape == times.shape == (3, 87)
    lens = [_padded_lengths(data, src[i], dst[i], times[i], P, L)[0] for i in range(3)]
    assert lens == want == [(4, 20), (4, 44), (8, 48)] and len(set(lens)) == 3
    N, G = src.shape
    assert (N * G, (N * G + 1) // 2) == (261, 131)
    # workgroup w holds pairs 2w and 2w + 1, pair b belongs to call b // G: an odd G puts a call boundary inside a workgroup
    straddling = [w for w in range((N * G + 1) // 2) if 2 * w + 1 < N * G and (2 * w) // G != (2 * w + 1) // G]
    assert G % 2 == 1 and straddling == [43]


def test_kernel_name_parser_of_the_dispatch_test():
    from tests.test_dygformer_large_batch_gpu import _instance
    assert _instance("void dygnn::v3::k_dygformer_fused3<4, true, 8, 0>(dygnn::v3::Args)") == ("k_dygformer_fused3", (4, 1, 8, 0))
    assert _instance("void dygnn::v3::k_dygformer_fused3<4, false, 4, 1>(dygnn::v3::Args) [clone .kd]") == ("k_dygformer_fused3", (4, 0, 4, 1))
    assert _instance("_ZN5dygnn2v318k_dygformer_fused3ILi4ELb1ELi8ELi0EEEvNS0_4ArgsE") == ("k_dygformer_fused3", (4, 1, 8, 0))
    assert _instance("void dygnn::v3::k_attn_bwd<4, 8>(dygnn::v3::AttnBwdArgs)") == ("k_attn_bwd", (4, 8))
    assert _instance("_ZN5dygnn2v39k_ffn_bwdILi8EEEvNS0_10FfnBwdArgsE.kd") == ("k_ffn_bwd", (8,))
    assert _instance("void at::native::vectorized_elementwise_kernel<4, ...>") is None
