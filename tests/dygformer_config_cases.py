"""DyGFormer across the configurations the library accepts: the recipes of tests/test_dygformer_configs_cpu.py (which asserts, without a
GPU, that every row is what its comment says) and tests/test_dygformer_configs_gpu.py (which holds the kernels to the CPU oracle on them).

The fused kernels (v3::supported, dygformer_fused3_pack.hip) take C = 50, H = 2, Fn / Fe / Ft multiples of 4 with Fn, Fe in 16..512 and
Ft in 16..216; everything else is the generic path (dygformer_generic.hip), which impl = 0 falls back to.  Training (train::supported,
dygformer_train.hip) takes C <= 51 and any H that divides 4 C.  One row per boundary of those ranges and per branch keyed on a dimension.
Inputs are a pure function of the row: nothing is stored."""
from __future__ import annotations

import functools

import numpy as np

from dyglib_amd import synthetic as syn

# label: (Fn, Fe, Ft, C, H, NL, P, L, B, node table, env) -- what each one crosses.  k-chunks of a projection channel = ceil(P F / 16); the
# fused kernels walk them in groups of four (GS) with remainder arms, and store them in slot groups of four (proj_slots).
CONFIGS = {
    # the smallest fused dims: ONE k-chunk per gathered channel and for the time channel (fewer than a slot group of four: remainder arm 1
    # only, three padding slots); the gather and time cursors wrap on every chunk (F = 16); the output layer is one 16-column tile; one layer
    "f16": (16, 16, 16, 50, 2, 1, 1, 32, 12, "dense", {}),
    # a patch size that is no power of two, L no multiple of P (padded lengths 33 = 11 tokens a side); F % 16 of 4 (node) and 8 (edge,
    # time): the time cursor wraps mid-row; chunks 4 / 8 / 5 (time: remainder arm 1); the output layer's last tile has 4 live columns
    "p3_ft24": (20, 40, 24, 50, 2, 2, 3, 31, 12, "dense", {}),
    # the same with the node table all zero: DYGNN_TABLE_NODE_ZERO skips the node channel, layer 0's Q/K/V take the constant-channel term
    "p3_ft24_zero": (20, 40, 24, 50, 2, 2, 3, 31, 12, "zero", {}),
    # the upper bounds of v3::supported: LDS exactly full at Ft = 216 ((38928 + 1600 + 432) * 4 = 160 KiB), 32 output tiles, P Fn = 1024
    # (64 node chunks), 27 time chunks (remainder arm 3), 22 edge chunks (arm 2); three layers
    "max_dims": (512, 172, 216, 50, 2, 3, 2, 64, 6, "dense", {}),
    # DYGNN_MAX_LAYERS layers; training: 4 * 8 + 4 = 36 weight-gradient problems in the grouped launch
    "l8": (172, 172, 100, 50, 2, 8, 4, 48, 4, "zero", {}),
    # more than 256 pairs: the eight-wave two-pair kernels at non-default dims, an odd batch (the last workgroup holds one pair); also run
    # with DYGNN_POOLED_TAIL=1 (k_pooled_tail: two 16-column output tiles) and DYGNN_PACK_PAIRS=1 (the packed kernel), both read per call
    "two_pair_f32": (32, 48, 24, 50, 2, 2, 2, 32, 261, "dense", {}),
    # one step past the fused bound on Fn: impl = 0 must take the generic path, impl = 3 must refuse
    "fn516": (516, 172, 100, 50, 2, 2, 2, 64, 6, "dense", {}),
    # one step past the fused bound on Ft (the LDS budget)
    "ft220": (172, 172, 220, 50, 2, 2, 2, 64, 6, "zero", {}),
    # Ft % 4 != 0: generic inference.  In training the time rows hold P Ft = 36 floats, still a multiple of 4: the time projection's
    # weight gradient stays in the grouped launch (DwList::try_add looks at P F, not at F; ft18_p1 below leaves it)
    "ft18": (172, 172, 18, 50, 2, 2, 2, 64, 6, "zero", {}),
    # D = 200 as in the fused kernel but five heads of 40: generic inference; training product by product with strides of hd = 40
    "h5": (172, 172, 100, 50, 5, 2, 2, 64, 6, "zero", {}),
    # D = 128, hd = 32: the generic kernels at another model width; Fe = 36 and Ft = 28 are multiples of 4 but not of 8
    "c32_h4": (20, 36, 28, 32, 4, 1, 2, 32, 12, "dense", {}),
    # everything odd: D = 52, Cp = 16 != C = 13 (the training path's channel split pads, a_kpad), one head, Fe = 1, Fn = 5, Ft = 7 (no
    # projection is 16-byte aligned: all four weight gradients leave the grouped launch), three layers
    "c13_h1": (5, 1, 7, 13, 1, 3, 1, 16, 9, "dense", {}),
    # training's upper bound (5 C = 255 <= 256), odd hd = 51, Cp = 52 != C
    "c51_h4": (172, 172, 100, 51, 4, 2, 4, 48, 10, "zero", {}),
    # D = 256, hd = 32: inference only, training must report unsupported (C > 51)
    "c64_h8": (172, 172, 100, 64, 8, 2, 2, 64, 10, "zero", {}),
    # (a row's seeds follow from its position: new rows go here, at the end)
    # ft18 with P = 1: rows of P Ft = 18 (time) and P C = 50 (co-occurrence) floats are not 16-byte aligned, so those two weight
    # gradients take the general GEMM (grouped[ch] == false) while node and edge stay in the grouped launch
    "ft18_p1": (172, 172, 18, 50, 2, 2, 1, 32, 6, "zero", {}),
}

FUSED = ("f16", "p3_ft24", "p3_ft24_zero", "max_dims", "l8", "two_pair_f32")         # rows v3::supported takes
UNTRAINABLE = ("c64_h8",)                                                             # rows train::supported refuses
# the env settings two_pair_f32 also runs under
EXTRA_ENV = {"two_pair_f32": ({"DYGNN_POOLED_TAIL": "1"}, {"DYGNN_PACK_PAIRS": "1"})}
# what the comments above claim, asserted by tests/test_dygformer_configs_cpu.py: padded lengths (S_src, S_dst) of the batch ...
PADDED = {"f16": (32, 32), "p3_ft24": (33, 33), "p3_ft24_zero": (33, 33), "max_dims": (64, 64), "l8": (48, 48), "two_pair_f32": (32, 32),
          "fn516": (64, 64), "ft220": (64, 64), "ft18": (64, 64), "ft18_p1": (32, 32), "h5": (64, 64), "c32_h4": (32, 32), "c13_h1": (16, 16), "c51_h4": (48, 48),
          "c64_h8": (64, 64)}
# ... and the k-chunk counts (node, edge, time) of the fused rows
CHUNKS = {"f16": (1, 1, 1), "p3_ft24": (4, 8, 5), "p3_ft24_zero": (4, 8, 5), "max_dims": (64, 22, 27), "l8": (43, 43, 25), "two_pair_f32": (4, 6, 3)}

NINE_LAYERS = "l8"          # the row whose dims the nine-layer rejection test takes


def dims(label: str) -> dict:
    Fn, Fe, Ft, C, H, NL, P, L, B, table, env = CONFIGS[label]
    return dict(Fn=Fn, Fe=Fe, Ft=Ft, C=C, H=H, NL=NL, P=P, L=L, B=B, table=table, env=env, D=4 * C, hd=4 * C // H)


def _seed(label: str) -> int:
    base = label[:-len("_zero")] if label.endswith("_zero") else label         # a "_zero" row shares everything but the node table
    return 70 + 3 * list(CONFIGS).index(base)


@functools.lru_cache(maxsize=None)
def build(label: str, num_layers: int = 0) -> dict:
    """-> the case dict tests.test_dygformer_gpu.build_model and the oracle harness of tests/test_train_gpu.py take: a bipartite graph (75
    nodes, 1500 interactions, every fifth timestamp a duplicate); the batch = the last B interactions, the first three moved to the
    earliest timestamp (empty histories).  num_layers > 0 overrides the row's.  Cached: treat the result as read-only."""
    d = dims(label)
    NL = num_layers or d["NL"]
    seed = _seed(label)
    data, _, ef = syn.make_bipartite_graph(60, 15, 1500, seed=seed, time_span=2.68e6, edge_feat_dim=d["Fe"], duplicate_time_every=5)
    nf = np.zeros((data.max_node_id + 1, d["Fn"]), dtype=np.float32)
    if d["table"] == "dense":
        nf[1:] = 0.5 * np.random.RandomState(seed + 1).standard_normal((data.max_node_id, d["Fn"])).astype(np.float32)
    E, B = data.num_interactions, d["B"]
    src, dst, t = data.src_node_ids[E - B:].copy(), data.dst_node_ids[E - B:].copy(), data.node_interact_times[E - B:].copy()
    t[:3] = data.node_interact_times.min()
    params = syn.make_dygformer_params(seed + 2, node_feat_dim=d["Fn"], edge_feat_dim=d["Fe"], time_feat_dim=d["Ft"],
                                       channel_embedding_dim=d["C"], patch_size=d["P"], num_layers=NL)
    cfg = dict(patch_size=d["P"], max_input_sequence_length=d["L"], num_heads=d["H"], num_layers=NL, time_feat_dim=d["Ft"],
               channel_embedding_dim=d["C"])
    return dict(data=data, node_feat=nf, edge_feat=ef, params=params, mparams=syn.make_merge_layer_params(seed + 1000), src=src, dst=dst,
                neg_dst=dst, times=t, cfg=cfg)


def capi_config(label: str, num_layers: int = 0):
    """the row as the library's dygnn_dygformer_config"""
    from dyglib_amd import _capi
    d = dims(label)
    return _capi.DygformerConfig(d["Fn"], d["Fe"], d["Ft"], d["C"], d["P"], num_layers or d["NL"], d["H"], d["L"])
