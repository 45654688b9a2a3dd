"""Seeded recipes for calls of MORE than kSmallBatchPairs (256) pairs: the sizes at which the fused DyGFormer path leaves its four-wave,
one-pair-per-workgroup kernels for the eight-wave ones (two pairs per workgroup, (B + 1) / 2 workgroups; k_ffn_bwd<8> on 128 dense token rows
per workgroup once a call has more than 64 * 256 of them).  Inputs are never stored: every recipe is a pure function of its seeds and returns

    data, node_feat, edge_feat, params, (src, dst, times)

tests/test_dygformer_large_batch_cases_cpu.py asserts, through the oracle's taps and without a GPU, the properties each docstring states —
the GPU tests rely on them to reach the kernel instances they are about."""
from __future__ import annotations

import numpy as np

from dyglib_amd import synthetic as syn
from tests import golden_cases as gc


def _head_and_tail(data, B: int, head: int = 3):
    """the first `head` interactions (empty histories) followed by the last B - head"""
    E = data.num_interactions
    idx = np.concatenate([np.arange(head), np.arange(E - (B - head), E)])
    return data.src_node_ids[idx].copy(), data.dst_node_ids[idx].copy(), data.node_interact_times[idx].copy()


def _nonzero_node_features(node_feat: np.ndarray, seed: int) -> np.ndarray:
    """row 0 (the padding node) stays zero; every other row 0.3 N(0, 1): the node-projection gradients are not trivially zero"""
    nf = node_feat.copy()
    nf[1:] = np.random.RandomState(seed).standard_normal(nf[1:].shape).astype(np.float32) * 0.3
    return nf


def full64(B: int = 257):
    """P = 2, L = 64, every late window full: padded lengths (64, 64), T = 64 tokens per pair — one pair fills the four token tiles of a
    wave quad exactly.  B = 257: the last eight-wave workgroup holds ONE pair, M = 16448 > 16384 dense rows, and k_ffn_bwd<8>'s last
    workgroup has 64 of its 128 rows."""
    data, nf, ef = syn.make_bipartite_graph(600, 80, 20000, seed=21, duplicate_time_every=5)
    return data, _nonzero_node_features(nf, 2), ef, syn.make_dygformer_params(121, patch_size=2), _head_and_tail(data, B)


def ragged40(B: int = 411):
    """P = 2, L = 40: padded lengths (40, 40), T = 40 — a token tile holds rows of both sides and the last tile of a pair is half empty.
    B = 411: M = 16440 > 16384 and 16440 mod 128 = 56, so in k_ffn_bwd<8>'s last workgroup wave 3 has 8 valid rows of 16 and waves 4-7 none."""
    data, nf, ef = syn.make_bipartite_graph(60, 8, 3000, seed=45, duplicate_time_every=5)
    return data, _nonzero_node_features(nf, 3), ef, syn.make_dygformer_params(145, patch_size=2), _head_and_tail(data, B)


def hub14(B: int = 257):
    """graph and parameters of golden_cases' hub_p4_l48 (P = 4, L = 48; low-degree users against 5 hub items), the last 257 of its 300
    interactions: padded lengths (8, 48), T = 14 — not a multiple of 4 (k_attn_bwd's scalar path) and below one 16-row tile.
    M = 3598 <= 16384: eight-wave forward and attention backward, FOUR-wave FFN backward."""
    c = gc.build_case("hub_p4_l48")
    d = c["data"]
    E = d.num_interactions
    idx = np.arange(E - B, E)
    return d, c["node_feat"], c["edge_feat"], c["params"], (d.src_node_ids[idx].copy(), d.dst_node_ids[idx].copy(), d.node_interact_times[idx].copy())


HUB_GROUP_ROWS = ((0, 87), (100, 187), (213, 300))


def hub_groups():
    """inference only: the hub graph as THREE calls of 87 pairs, [3, 87] arrays (interactions 0..86, 100..186, 213..299) with padded lengths
    (4, 20), (4, 44), (8, 48).  One grouped launch: 261 pairs in 131 two-pair workgroups (workgroup w holds pairs 2w and 2w + 1).  The
    group size is odd, so the boundary at pair 87 falls INSIDE workgroup 43: it holds the last pair of call 0 and the first pair of call 1,
    each with its own padded lengths.  (The boundary at pair 174 is even: workgroup 86 ends call 1, workgroup 87 starts call 2.)"""
    c = gc.build_case("hub_p4_l48")
    d = c["data"]
    rows = [np.arange(a, b) for a, b in HUB_GROUP_ROWS]
    batch = tuple(np.stack([arr[r] for r in rows]) for arr in (d.src_node_ids, d.dst_node_ids, d.node_interact_times))
    return d, c["node_feat"], c["edge_feat"], c["params"], batch


# name -> (recipe, patch size, max_input_sequence_length, padded lengths (S_src, S_dst) of every call)
RECIPES = {
    "full64": (full64, 2, 64, [(64, 64)]),
    "ragged40": (ragged40, 2, 40, [(40, 40)]),
    "hub14": (hub14, 4, 48, [(8, 48)]),
    "hub_groups": (hub_groups, 4, 48, [(4, 20), (4, 44), (8, 48)]),
}


def build(name: str, *args, num_layers: int = 2, params=None) -> dict:
    """the recipe as the case dict of golden_cases.build_case (what tests.test_dygformer_gpu.build_model and the oracle-autograd harness
    of tests.test_train_gpu take); `seq_lens` = the padded lengths the recipe promises"""
    fn, P, L, lens = RECIPES[name]
    data, nf, ef, p, (src, dst, times) = fn(*args)
    cfg = dict(patch_size=P, max_input_sequence_length=L, num_heads=2, num_layers=num_layers, time_feat_dim=100, channel_embedding_dim=50)
    return dict(data=data, node_feat=nf, edge_feat=ef, params=p if params is None else params, mparams=syn.make_merge_layer_params(1121),
                src=src, dst=dst, times=times, cfg=cfg, seq_lens=lens)
