"""No GPU: every row of tests/dygformer_config_cases.py is what its comment says (padded lengths, empty histories, which paths the library's
host-side queries give it, k-chunk counts, magnitudes), and the oracle's training-path dropout (oracle/dygformer_oracle.py TrainDropout)
draws the masks dropout.h documents."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import dropout as odrop
from oracle import dygformer_oracle as orc
from oracle import tgat_oracle as torc
from tests import dygformer_config_cases as cc

SEED = (5 << 40) + 12345


@functools.lru_cache(maxsize=None)
def _oracle(label, p=None, seed=SEED):
    """(src emb, dst emb, taps, the TrainDropout or None) of the row; p = None: the plain oracle"""
    d, c = cc.dims(label), cc.build(label)
    g = c["data"]
    adj = orc.OracleAdjacency(g.src_node_ids, g.dst_node_ids, g.edge_ids, g.node_interact_times)
    taps = {}
    extra = {} if p is None else {"dropout": orc.TrainDropout(p, seed)}
    with torch.no_grad():
        s, t = orc.dygformer_forward(c["params"], c["node_feat"], c["edge_feat"], adj, c["src"], c["dst"], c["times"], d["P"], d["L"], d["H"], d["NL"],
                                     taps=taps, **extra)
    return s.numpy(), t.numpy(), taps, extra.get("dropout")


def _lib():
    from dyglib_amd import _capi
    return _capi.load()


def test_the_rows_the_issue_names_are_all_present():
    assert set(cc.CONFIGS) >= {"f16", "p3_ft24", "p3_ft24_zero", "max_dims", "l8", "two_pair_f32", "fn516", "ft220", "ft18", "h5", "c32_h4", "c13_h1",
                               "c51_h4", "c64_h8"}
    assert set(cc.FUSED) <= set(cc.CONFIGS) and set(cc.UNTRAINABLE) <= set(cc.CONFIGS) and set(cc.PADDED) == set(cc.CONFIGS)
    assert set(cc.CHUNKS) == set(cc.FUSED)
    assert cc.CONFIGS["p3_ft24"][:9] == cc.CONFIGS["p3_ft24_zero"][:9]
    a, b = cc.build("p3_ft24"), cc.build("p3_ft24_zero")
    assert all(np.array_equal(a["params"][k], b["params"][k]) for k in a["params"]) and np.array_equal(a["src"], b["src"])


@pytest.mark.parametrize("label", list(cc.CONFIGS))
def test_batch_and_tables_are_what_the_row_says(label):
    d, c = cc.dims(label), cc.build(label)
    _, _, taps, _ = _oracle(label)
    assert len(c["src"]) == d["B"] and c["node_feat"].shape[1] == d["Fn"] and c["edge_feat"].shape[1] == d["Fe"]
    # padded lengths, from the oracle's taps and from the definition (models/DyGFormer.py:214-226) on the raw interaction list
    assert (taps["src_ids"].shape[1], taps["dst_ids"].shape[1]) == cc.PADDED[label]
    g = c["data"]
    for ids, S in ((c["src"], cc.PADDED[label][0]), (c["dst"], cc.PADDED[label][1])):
        hist = [int((((g.src_node_ids == n) | (g.dst_node_ids == n)) & (g.node_interact_times < t)).sum()) for n, t in zip(ids, c["times"])]
        longest = min(max(hist), d["L"] - 1) + 1
        assert S == -(-longest // d["P"]) * d["P"]
    assert (cc.PADDED[label][0] % d["P"], d["L"] % d["P"] != 0) == (0, label.startswith("p3_ft24"))
    # empty histories: the first three pairs, on both sides
    for side in ("src_ids", "dst_ids"):
        empty = (taps[side][:, 1:] == 0).all(axis=1)
        assert empty[:3].all() and not empty[3:].any(), (label, side)
    # node table: all zero, or dense with the padding row zero
    if d["table"] == "zero":
        assert not c["node_feat"].any()
    else:
        assert not c["node_feat"][0].any() and (c["node_feat"][1:] != 0).all()
    assert not c["edge_feat"][0].any() and c["edge_feat"][1:].any()


@pytest.mark.parametrize("label", list(cc.CONFIGS))
def test_host_queries_classify_the_row_as_labelled(label):
    d = cc.dims(label)
    lib, cfg = _lib(), cc.capi_config(label)
    fused = lib.dygnn_dygformer_projected_bytes(C.byref(cfg), 10) > 0
    assert fused == (label in cc.FUSED)
    # the bounds as the row comments state them
    want_fused = (d["C"] == 50 and d["H"] == 2 and all(d[k] % 4 == 0 and d[k] >= 16 for k in ("Fn", "Fe", "Ft")) and d["Fn"] <= 512 and
                  (38928 + 1600 + 2 * d["Ft"]) * 4 <= 160 * 1024)
    assert fused == want_fused
    trainable = lib.dygnn_dygformer_train_workspace_bytes(C.byref(cfg), d["B"]) > 0
    assert trainable == (label not in cc.UNTRAINABLE) == (d["C"] <= 51)
    assert lib.dygnn_dygformer_packed_bytes(C.byref(cfg)) > 0 and lib.dygnn_dygformer_workspace_bytes_for(C.byref(cfg), d["B"], 1) > 0
    assert (lib.dygnn_dygformer_workspace_bytes_for(C.byref(cfg), d["B"], 0) > 0)


def test_row_specific_claims():
    d = cc.dims
    assert (38928 + 1600 + 2 * d("max_dims")["Ft"]) * 4 == 160 * 1024 and d("max_dims")["Fn"] == 512 and (d("max_dims")["Fn"] + 15) // 16 == 32
    assert d("max_dims")["P"] * d("max_dims")["Fn"] == 1024
    assert (d("f16")["Fn"] + 15) // 16 == 1 and d("f16")["NL"] == 1
    assert d("p3_ft24")["Fn"] % 16 == 4 and d("p3_ft24")["Fe"] % 16 == 8 and d("p3_ft24")["Ft"] % 16 == 8
    assert d("l8")["NL"] == 8 and 4 * d("l8")["NL"] + 4 == 36
    assert d("two_pair_f32")["B"] > 256 and d("two_pair_f32")["B"] % 2 == 1 and 2 * cc.PADDED["two_pair_f32"][0] // d("two_pair_f32")["P"] <= 64
    assert d("fn516")["Fn"] == 512 + 4 and d("ft220")["Ft"] == 216 + 4 and d("ft18")["Ft"] % 4 != 0
    # which projection weight gradients join the grouped launch (DwList::try_add: rows of P F floats, 16-byte aligned or not)
    grouped = lambda r: tuple((r["P"] * r[k]) % 4 == 0 for k in ("Fn", "Fe", "Ft", "C"))
    assert grouped(d("ft18")) == (True, True, True, True) and grouped(d("ft18_p1")) == (True, True, False, False)
    assert grouped(d("c13_h1")) == (False, False, False, False) and grouped(d("l8")) == (True, True, True, True)
    assert (d("h5")["D"], d("h5")["hd"]) == (200, 40) and (d("c32_h4")["D"], d("c32_h4")["hd"]) == (128, 32)
    c13 = d("c13_h1")
    assert (c13["D"], c13["H"], (c13["C"] + 3) & ~3, c13["NL"], c13["Fe"]) == (52, 1, 16, 3, 1)
    assert all((c13["P"] * c13[k]) % 4 != 0 for k in ("Fn", "Fe", "Ft", "C"))
    assert 5 * d("c51_h4")["C"] == 255 and d("c51_h4")["hd"] == 51 and (d("c64_h8")["D"], d("c64_h8")["hd"]) == (256, 32)


@pytest.mark.parametrize("label", list(cc.FUSED))
def test_chunk_counts_of_the_fused_rows(label):
    d = cc.dims(label)
    chunks = tuple(-(-d["P"] * d[k] // 16) for k in ("Fn", "Fe", "Ft"))
    assert chunks == cc.CHUNKS[label]
    residues = {"f16": (1, 1, 1), "p3_ft24": (0, 0, 1), "p3_ft24_zero": (0, 0, 1), "max_dims": (0, 2, 3), "l8": (3, 3, 1), "two_pair_f32": (0, 2, 3)}
    assert tuple(n % 4 for n in chunks) == residues[label]


def test_the_fused_rows_reach_every_remainder_arm_in_every_channel_kind():
    """n % GS of 1, 2 and 3 in a gathered channel (node or edge) and in the time channel, over the fused rows together"""
    gathered = {n % 4 for label in cc.FUSED for n in cc.CHUNKS[label][:2]}
    timed = {cc.CHUNKS[label][2] % 4 for label in cc.FUSED}
    assert gathered >= {0, 1, 2, 3} and timed >= {1, 3}


@pytest.mark.parametrize("label", list(cc.CONFIGS))
def test_magnitudes_stay_where_the_bars_are_meant_for(label):
    s, t, taps, _ = _oracle(label)
    assert max(np.abs(s).max(), np.abs(t).max()) <= 20
    assert max(float(x.abs().max()) for x in [taps["encoder_input"]] + taps["layer_outputs"]) <= 140


def test_nine_layers_are_refused_by_the_host_check():
    lib, cfg = _lib(), cc.capi_config(cc.NINE_LAYERS, 9)
    assert lib.dygnn_dygformer_packed_bytes(C.byref(cfg)) == 0
    assert b"num_layers" in lib.dygnn_last_error()


# ---- the oracle's dropout ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("label", ["c32_h4", "c13_h1", "p3_ft24"])
def test_dropout_oracle_at_p0_is_the_plain_oracle_bit_for_bit(label):
    s0, t0, taps0, _ = _oracle(label)
    s1, t1, taps1, _ = _oracle(label, 0.0)
    assert np.array_equal(s0, s1) and np.array_equal(t0, t1)
    for a, b in zip(taps0["layer_outputs"], taps1["layer_outputs"]):
        assert torch.equal(a, b)


def test_dropout_oracle_drops_a_tenth_of_every_site():
    """p = 0.1 at c32_h4: every site's dropped share is 0.1 +- 0.02 (so its kept share 0.9 +- 0.02), kept elements carry float32 1/(1-p)"""
    s0, _, _, _ = _oracle("c32_h4")
    s1, _, _, dr = _oracle("c32_h4", 0.1)
    assert sorted(dr.dropped) == [0, 1, 2, 3]                 # one layer: sites 4 * 0 + {0, 1, 2, 3}
    for site, share in dr.dropped.items():
        assert abs(share - 0.1) <= 0.02, (site, share)
    m = orc.TrainDropout(0.1, SEED).mask(2, (3, 5, 7)).numpy()
    assert set(np.unique(m).tolist()) <= {0.0, float(np.float32(1.0 / (1.0 - float(np.float32(0.1)))))}
    assert not np.array_equal(s0, s1)


def test_dropout_masks_index_the_dense_row_major_tensor_of_the_site():
    """site 4 l + 0 at ((b H + h) T + q) T + k, the others at (b T + tok) W + j: the mask of a shape is the generator at those offsets"""
    dr = orc.TrainDropout(0.1, SEED)
    B, H, T, D = 3, 5, 7, 20
    m = dr.mask(4 * 2 + 0, (B, H, T, T)).numpy()
    for b, h, q, k in ((0, 0, 0, 0), (1, 3, 2, 6), (2, 4, 6, 6)):
        assert m[b, h, q, k] == odrop.mask(0.1, SEED, 8, ((b * H + h) * T + q) * T + k)
    for site, W in ((1, D), (2, 4 * D), (3, D)):
        m = dr.mask(site, (B, T, W)).numpy()
        for b, tok, j in ((0, 0, 0), (1, 4, W - 1), (2, 6, 3)):
            assert m[b, tok, j] == odrop.mask(0.1, SEED, site, (b * T + tok) * W + j)


def test_dropout_seed_high_word_reaches_the_masks():
    a = orc.TrainDropout(0.1, (5 << 40) + 12345).mask(0, (4096,)).numpy()
    b = orc.TrainDropout(0.1, (6 << 40) + 12345).mask(0, (4096,)).numpy()
    assert not np.array_equal(a, b)
    sa, _, _, _ = _oracle("c32_h4", 0.1, (5 << 40) + 12345)
    sb, _, _, _ = _oracle("c32_h4", 0.1, (6 << 40) + 12345)
    assert not np.array_equal(sa, sb)


def _mix32(x):
    x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF; x ^= x >> 16
    return x


def test_dropout_generator_is_the_one_of_the_tgat_oracle_and_of_dropout_h():
    """One generator for every backbone's oracle: the same (p, seed, site, index) gives the same multiplier through either TrainDropout, and
    both equal dropout.h's arithmetic written out in Python integers"""
    p = 0.1
    a, b = orc.TrainDropout(p, SEED), torc.TrainDropout(p, SEED)
    assert type(a.gen) is type(b.gen) is odrop.Drop
    thresh = int(float(np.float32(p)) * 4294967296.0)
    scale = np.float32(1.0 / (1.0 - float(np.float32(p))))
    key0, key1 = SEED & 0xFFFFFFFF, ((SEED >> 32) * 0x85EBCA6B + 0x165667B1) & 0xFFFFFFFF
    for site, idx in ((0, 0), (1, 1), (3, 12345), (7, 2 ** 31 + 5), (30, 2 ** 32 - 1), (2, 2 ** 32 + 9), (5, 3 * 2 ** 32 + 77)):
        want = a.gen.mask(site, np.array([idx], dtype=np.int64))[0]
        assert want == b.gen.mask(site, np.array([idx], dtype=np.int64))[0]
        skey = _mix32((key0 + 0x9E3779B9 * (site + 1)) & 0xFFFFFFFF) ^ key1
        folded = ((idx & 0xFFFFFFFF) + 0x27D4EB2F * (idx >> 32)) & 0xFFFFFFFF
        assert want == (scale if _mix32(folded ^ skey) >= thresh else np.float32(0.0)), (site, idx)
