"""CPU-only checks of the boundary: the C-ABI library builds, loads and exports every symbol
include/dygnn.h declares; the host CSR builder matches the oracle; argument validation maps to the
reference's exception types; the nn.Module mirrors carry the reference's state_dict keys.
No kernel is launched here."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import torch

from dyglib_amd import _build, _capi, synthetic as syn
from dyglib_amd.temporal_csr import TemporalCSR
from oracle import dygformer_oracle as orc
from tests import golden_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    _build.build(verbose=False)          # hipcc cross-compiles gfx950 without a GPU
    return _capi.load()


def test_header_symbols_are_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "dygnn.h")).read()
    declared = set(re.findall(r"\b(dygnn_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    assert declared == set(_capi.SIGNATURES), (declared ^ set(_capi.SIGNATURES))
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.dygnn_abi_version() == _capi.ABI_VERSION


def test_struct_layouts_match_header():
    assert C.sizeof(_capi.Csr) == 6 * 8
    assert C.sizeof(_capi.DygformerConfig) == 8 * 4
    assert C.sizeof(_capi.EncoderLayerWeights) == 12 * 8
    assert C.sizeof(_capi.DygformerWeights) == (14 + 12 * _capi.DYGNN_MAX_LAYERS + 2) * 8
    assert C.sizeof(_capi.DygformerTaps) == (5 + _capi.DYGNN_MAX_LAYERS) * 8
    assert C.sizeof(_capi.MmArgs) == 7 * 8 + 6 * 8 + 8 * 4 + 2 * 4 + 5 * 4 + 4           # 4 bytes of tail padding
    assert C.sizeof(_capi.DwPair) == 8 + 2 * 4 + 8 + 2 * 4 + 8 + 4 + 4 + 8               # 4 bytes of padding behind ldc


@pytest.mark.parametrize("name", ["bip_p2_l64", "gen_p1_l32"])
def test_csr_host_builder_matches_oracle(lib, name):
    d = gc.build_case(name)["data"]
    csr = TemporalCSR.from_interactions(d.src_node_ids, d.dst_node_ids, d.edge_ids, d.node_interact_times)
    adj = orc.OracleAdjacency(d.src_node_ids, d.dst_node_ids, d.edge_ids, d.node_interact_times)
    np.testing.assert_array_equal(csr.indptr, adj.indptr)
    np.testing.assert_array_equal(csr.nbr, adj.nbr)
    np.testing.assert_array_equal(csr.eid, adj.eid)
    np.testing.assert_array_equal(csr.ts, adj.ts)
    assert csr.indptr[1] == 0                                  # row 0 = padding node, empty
    # reference constructor input (adj_list of tuples, utils/utils.py:297-300) gives the same CSR
    adj_list = [[] for _ in range(d.max_node_id + 1)]
    for s, t, e, ts in zip(d.src_node_ids, d.dst_node_ids, d.edge_ids, d.node_interact_times):
        adj_list[s].append((t, e, ts))
        adj_list[t].append((s, e, ts))
    csr2 = TemporalCSR.from_adj_list(adj_list)
    for f in ("indptr", "nbr", "eid", "ts"):
        np.testing.assert_array_equal(getattr(csr, f), getattr(csr2, f))


def test_csr_builder_edge_cases(lib):
    # empty interaction list: only the padding row
    e = np.zeros(0, dtype=np.int64)
    csr = TemporalCSR.from_interactions(e, e, e, np.zeros(0))
    assert csr.num_nodes == 1 and csr.num_entries == 0
    # out-of-range node id -> IndexError like the reference's adj_list[...] indexing
    with pytest.raises(IndexError):
        TemporalCSR.from_interactions(np.array([5]), np.array([1]), np.array([1]), np.array([0.0]), num_nodes=3)
    # self interaction: stored twice under the same node, src entry first
    csr = TemporalCSR.from_interactions(np.array([2, 2]), np.array([2, 1]), np.array([1, 2]), np.array([1.0, 1.0]))
    assert csr.nbr[csr.indptr[2]:csr.indptr[3]].tolist() == [2, 2, 1]
    assert csr.eid[csr.indptr[2]:csr.indptr[3]].tolist() == [1, 1, 2]


def test_argument_validation_without_gpu(lib):
    csr = _capi.Csr(1, 0, 1, None, None, None)    # non-null dummy indptr; never dereferenced (rejected before launch)
    rc = lib.dygnn_sample_recent(C.byref(csr), None, None, 4, 0, None, None, None, None)
    assert rc == -1 and b"greater than 0" in lib.dygnn_last_error()               # utils/utils.py:157
    with pytest.raises(AssertionError):
        _capi.check(rc)
    rc = lib.dygnn_window_lengths(C.byref(csr), None, None, 0, 1, None, None, None, None)
    assert rc == -1 and b"greater than 1" in lib.dygnn_last_error()               # models/DyGFormer.py:209
    cfg = _capi.DygformerConfig(172, 172, 100, 50, 2, 2, 3, 64)                   # 200 % 3 != 0
    assert lib.dygnn_dygformer_packed_bytes(C.byref(cfg)) == 0
    cfg = _capi.DygformerConfig(172, 172, 100, 50, 2, 2, 2, 64)
    assert lib.dygnn_dygformer_packed_bytes(C.byref(cfg)) > 4_000_000                # ~ one copy of the weight matrices
    assert lib.dygnn_dygformer_workspace_bytes(C.byref(cfg), 200) > 0


def test_module_state_dict_matches_reference_keys(lib):
    from dyglib_amd import DyGFormer, MergeLayer, NeighborSampler
    data, nf, ef = syn.make_bipartite_graph(5, 3, 20, seed=0)
    sampler = NeighborSampler(None, "recent", seed=0, csr=TemporalCSR.from_interactions(
        data.src_node_ids, data.dst_node_ids, data.edge_ids, data.node_interact_times), device="cpu")
    m = DyGFormer(nf, ef, sampler, time_feat_dim=100, channel_embedding_dim=50, patch_size=2, num_layers=2, num_heads=2,
                  dropout=0.1, max_input_sequence_length=64, device="cpu")
    want = syn.dygformer_param_shapes(172, 172, 100, 50, 2, 2)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == want
    assert sum(int(np.prod(s)) for s in got.values()) == 1_052_222
    # golden parameter sets load strictly
    m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.make_dygformer_params(3, patch_size=2).items()}, strict=True)
    ml = MergeLayer(172, 172, 172, 1)
    assert {k: tuple(v.shape) for k, v in ml.state_dict().items()} == {
        "fc1.weight": (172, 344), "fc1.bias": (172,), "fc2.weight": (1, 172), "fc2.bias": (1,)}
    # time encoder init = reference's 10^-linspace(0,9,100), bias 0 (models/modules.py:20-21)
    np.testing.assert_allclose(m2 := DyGFormer(nf, ef, sampler, 100, 50).time_encoder.w.weight.detach().numpy().ravel(),
                               1 / 10 ** np.linspace(0, 9, 100, dtype=np.float32))
    # no silent CPU path: a CPU-resident model refuses to run
    with pytest.raises(_capi.DygnnError):
        m.eval()
        with torch.no_grad():
            m.compute_src_dst_node_temporal_embeddings(data.src_node_ids[:2], data.dst_node_ids[:2], data.node_interact_times[:2])
    # the training path is HIP too: a CPU-resident model refuses it the same way
    m.train()
    with pytest.raises(_capi.DygnnError):
        m.compute_src_dst_node_temporal_embeddings(data.src_node_ids[:2], data.dst_node_ids[:2], data.node_interact_times[:2])


def test_unsupported_sampling_strategies_raise(lib):
    from dyglib_amd import NeighborSampler
    data, _, _ = syn.make_bipartite_graph(5, 3, 20, seed=0)
    csr = TemporalCSR.from_interactions(data.src_node_ids, data.dst_node_ids, data.edge_ids, data.node_interact_times)
    s = NeighborSampler(None, "uniform", seed=1, csr=csr, device="cpu")
    assert s.seed == 1 and s.sample_neighbor_strategy == "uniform"
    s.reset_random_state()
    with pytest.raises(NotImplementedError):
        s._require_recent()
    with pytest.raises(ValueError):
        NeighborSampler(None, "bogus", csr=csr, device="cpu")._require_recent()


# ---- TGAT / TGN / TGAT training: workspace sizes and argument validation -----------------------------------------------------------------
# Callers size their workspaces with these functions, so their values are part of the interface: pinned over a grid of configs.
WS_GRID = list(itertools.product((1, 2, 3), (1, 10, 20, 64), (1, 2), ((172, 172, 100), (16, 16, 16)), (1, 200)))   # L, k, H, (Fn, Fe, Ft), batch
TGN_NODES = (100, 9228)
TGAT_WS = [
    3721728, 8137984, 44800, 545024, 3803648, 9633536, 45312, 698624, 3721728, 8209920, 44800, 616960, 3803648, 9705472, 45312, 770560, 3721984,
    8289792, 45056, 696832, 3803904, 9785344, 45568, 850432, 3723776, 8641792, 46848, 1048832, 3805696, 10137344, 47360, 1202432, 5758976,
    14897152, 78336, 1135872, 5922816, 17888256, 79872, 1443072, 5963008, 55821824, 104960, 6636544, 6190848, 71600128, 113152, 8326144,
    6197248, 102815488, 142592, 14270208, 6495744, 132801792, 158464, 17495808, 7325184, 328437760, 404736, 66708480, 7936512, 420939264,
    454400, 76692480, 7809280, 26322944, 103680, 2207744, 8061696, 32230400, 106752, 2822144, 10464000, 557410048, 444928, 70536448, 11547904,
    729551104, 537600, 89122048, 17878528, 2040353536, 1549568, 291463936, 21235712, 2667150592, 1888000, 359201536, 112317440, 20928110336,
    21464320, 4274414336, 142556160, 26931214592, 24708864, 4923374336
]
TGAT_TRAIN_WS = [
    56832, 10073600, 9984, 1152256, 71168, 12916736, 11008, 1460992, 56832, 10159872, 9984, 1238528, 71168, 13017344, 11008, 1561600, 57088,
    10255616, 10240, 1334272, 71680, 13129216, 11520, 1673472, 59136, 10678016, 12288, 1756672, 73984, 13622016, 13824, 2166272, 130048,
    24580096, 18944, 2802432, 165888, 31688704, 22528, 3575040, 588800, 116215040, 76032, 14149632, 753408, 149085184, 93696, 17874176, 1106432,
    219854592, 147968, 28581376, 1415168, 281652992, 183808, 35890176, 3501056, 698680320, 579584, 114891776, 4465664, 891563520, 713216,
    141771776, 277248, 53592832, 36864, 6101504, 355072, 69232640, 45056, 7802112, 6423040, 1282814464, 787200, 156165120, 8238336, 1645825280,
    991744, 197307136, 23115776, 4621421824, 3010048, 600756480, 29612032, 5920641024, 3777536, 754426880, 227103488, 45418785024, 37349888,
    7468628480, 289798400, 57957716224, 46086144, 9216084480
]
TGN_WS = [
    3861760, 16568576, 8278016, 20984832, 59904, 1374720, 560128, 1874944, 3943680, 16650496, 9773568, 22480384, 60416, 1375232, 713728,
    2028544, 3861760, 16568576, 8349952, 21056768, 59904, 1374720, 632064, 1946880, 3943680, 16650496, 9845504, 22552320, 60416, 1375232,
    785664, 2100480, 3862016, 16568832, 8429824, 21136640, 60160, 1374976, 711936, 2026752, 3943936, 16650752, 9925376, 22632192, 60672,
    1375488, 865536, 2180352, 3863808, 16570624, 8781824, 21488640, 61952, 1376768, 1063936, 2378752, 3945728, 16652544, 10277376, 22984192,
    62464, 1377280, 1217536, 2532352, 5899008, 18605824, 15037184, 27744000, 93440, 1408256, 1150976, 2465792, 6062848, 18769664, 18028288,
    30735104, 94976, 1409792, 1458176, 2772992, 6103040, 18809856, 55961856, 68668672, 120064, 1434880, 6651648, 7966464, 6330880, 19037696,
    71740160, 84446976, 128256, 1443072, 8341248, 9656064, 6337280, 19044096, 102955520, 115662336, 157696, 1472512, 14285312, 15600128,
    6635776, 19342592, 132941824, 145648640, 173568, 1488384, 17510912, 18825728, 7465216, 20172032, 328577792, 341284608, 419840, 1734656,
    66723584, 68038400, 8076544, 20783360, 421079296, 433786112, 469504, 1784320, 76707584, 78022400, 7949312, 20656128, 26462976, 39169792,
    118784, 1433600, 2222848, 3537664, 8201728, 20908544, 32370432, 45077248, 121856, 1436672, 2837248, 4152064, 10604032, 23310848, 557550080,
    570256896, 460032, 1774848, 70551552, 71866368, 11687936, 24394752, 729691136, 742397952, 552704, 1867520, 89137152, 90451968, 18018560,
    30725376, 2040493568, 2053200384, 1564672, 2879488, 291479040, 292793856, 21375744, 34082560, 2667290624, 2679997440, 1903104, 3217920,
    359216640, 360531456, 112457472, 125164288, 20928250368, 20940957184, 21479424, 22794240, 4274429440, 4275744256, 142696192, 155403008,
    26931354624, 26944061440, 24723968, 26038784, 4923389440, 4924704256
]


def test_tgat_tgn_workspace_sizes_are_pinned(lib):
    tgat, train, tgn = [], [], []
    for L, k, H, (fn, fe, ft), B in WS_GRID:
        cfg = _capi.TgatConfig(fn, fe, ft, L, H, k)
        tgat.append(lib.dygnn_tgat_workspace_bytes(C.byref(cfg), B))
        train.append(lib.dygnn_tgat_train_workspace_bytes(C.byref(cfg), B))
        tgn += [lib.dygnn_tgn_workspace_bytes(C.byref(cfg), N, B) for N in TGN_NODES]
    assert tgat == TGAT_WS
    assert train == TGAT_TRAIN_WS
    assert tgn == TGN_WS


# Every case below must be rejected before the entry point's first copy or launch, so the dummy device pointers are never used.  Were a check
# ever misplaced, a copy or a kernel would receive them: on a GPU machine that could fault a shared card, so these run on CPU machines only
# (where tests/test_sanitizers_cpu.py also runs them under ASan / UBSan).
cpu_only = pytest.mark.skipif(torch.cuda.is_available(), reason="hands dummy device pointers to the library: CPU machines only")
DUMMY = 1 << 20


def _weights(L, hole=None):
    w = _capi.TgatWeights(DUMMY, DUMMY)
    for l in range(L):
        for f, _ in _capi.TgatLayerWeights._fields_:
            setattr(w.layers[l], f, None if hole == (l, f) else DUMMY)
    return w


def _levels(L, hole=None):
    lv = _capi.TgatLevels()
    for l in range(L + 1):
        lv.ids[l] = None if hole == ("ids", l) else DUMMY
        if l:
            lv.nbr_eid[l] = None if hole == ("nbr_eid", l) else DUMMY
            lv.nbr_dt[l] = None if hole == ("nbr_dt", l) else DUMMY
    return lv


def _expect(lib, rc, code, fragment):
    assert rc == code, (rc, lib.dygnn_last_error())
    assert fragment in lib.dygnn_last_error().decode(), lib.dygnn_last_error()


@cpu_only
def test_tgat_inference_validates_before_any_hip_call(lib):
    L, B, D = 2, 3, DUMMY
    cfg = _capi.TgatConfig(16, 16, 16, L, 2, 4)
    csr = _capi.Csr(10, 10, D, D, D, D)
    need = lib.dygnn_tgat_workspace_bytes(C.byref(cfg), B)
    fwd = lambda w, nbytes: lib.dygnn_tgat_forward(C.byref(cfg), C.byref(w), C.byref(csr), D, D, D, D, D, B, D, D, D, nbytes, None)
    _expect(lib, fwd(_weights(L, (1, "fc2_b")), need), -1, "tgat: null layer weights (layer 1)")
    _expect(lib, fwd(_weights(L), need - 1), -4, "tgat: workspace too small")
    lvl = lambda w, lv, nbytes: lib.dygnn_tgat_forward_levels(C.byref(cfg), C.byref(w), C.byref(lv), D, D, B, D, D, D, nbytes, None)
    _expect(lib, lvl(_weights(L, (0, "query_w")), _levels(L), need), -1, "tgat: null layer weights (layer 0)")
    _expect(lib, lvl(_weights(L), _levels(L), need - 1), -4, "tgat: workspace too small")
    for hole in (("ids", 1), ("nbr_eid", 1), ("nbr_dt", 2), ("ids", 2)):
        _expect(lib, lvl(_weights(L), _levels(L, hole), need), -1, f"tgat: null level array (level {hole[1]})")
    roots = lambda w, nbytes: lib.dygnn_tgat_forward_roots(C.byref(cfg), C.byref(w), C.byref(csr), D, D, D, D, 2 * B, D, D, nbytes, None)
    _expect(lib, roots(_weights(L, (1, "key_w")), need), -1, "tgat: null layer weights (layer 1)")
    _expect(lib, roots(_weights(L), need - 1), -4, "tgat: workspace too small")
    # node + edge + time dims above 1024 (four float4 columns per lane in the attention kernels, the training path's bound too)
    wide, edge = _capi.TgatConfig(172, 756, 100, L, 2, 4), _capi.TgatConfig(172, 752, 100, L, 2, 4)
    assert lib.dygnn_tgat_workspace_bytes(C.byref(wide), B) == 0 and lib.dygnn_tgat_workspace_bytes(C.byref(edge), B) > 0
    assert lib.dygnn_tgat_train_workspace_bytes(C.byref(wide), B) == 0 and lib.dygnn_tgat_train_workspace_bytes(C.byref(edge), B) > 0
    too_wide = "tgat: node_feat_dim + edge_feat_dim + time_feat_dim > 1024 not supported"
    _expect(lib, lib.dygnn_tgat_forward(C.byref(wide), C.byref(_weights(L)), C.byref(csr), D, D, D, D, D, B, D, D, D, 1 << 40, None), -1, too_wide)
    _expect(lib, lib.dygnn_tgat_forward_levels(C.byref(wide), C.byref(_weights(L)), C.byref(_levels(L)), D, D, B, D, D, D, 1 << 40, None), -1, too_wide)
    _expect(lib, lib.dygnn_tgat_forward_roots(C.byref(wide), C.byref(_weights(L)), C.byref(csr), D, D, D, D, 2 * B, D, D, 1 << 40, None), -1, too_wide)


@cpu_only
def test_tgn_validates_before_any_hip_call(lib):
    L, B, N, D = 2, 3, 10, DUMMY
    cfg = _capi.TgatConfig(16, 16, 16, L, 2, 4)
    csr = _capi.Csr(N, 10, D, D, D, D)
    st = _capi.TgnState(N, D, D, D, D, D)
    gru = _capi.GruWeights(D, D, D, D)
    need = lib.dygnn_tgn_workspace_bytes(C.byref(cfg), N, B)
    step = lambda w, g, nbytes: lib.dygnn_tgn_forward_step(C.byref(cfg), C.byref(w), C.byref(g), C.byref(csr), D, D, C.byref(st), D, D, D, D, B, B,
                                                           D, D, D, nbytes, None)
    _expect(lib, step(_weights(L), _capi.GruWeights(D, D, None, D), need), -1, "tgn: null GRU weights")
    _expect(lib, step(_weights(L, (1, "ln_w")), gru, need), -1, "tgat: null layer weights (layer 1)")
    _expect(lib, step(_weights(L), gru, need - 1), -4, "tgn: workspace too small")
    lvl = lambda w, g, lv, nbytes: lib.dygnn_tgn_forward_levels(C.byref(cfg), C.byref(w), C.byref(g), C.byref(lv), D, D, C.byref(st), D, D, D, D, B, B,
                                                                D, D, D, nbytes, None)
    _expect(lib, lvl(_weights(L), _capi.GruWeights(None, D, D, D), _levels(L), need), -1, "tgn: null GRU weights")
    _expect(lib, lvl(_weights(L, (0, "res_b")), gru, _levels(L), need), -1, "tgat: null layer weights (layer 0)")
    _expect(lib, lvl(_weights(L), gru, _levels(L), need - 1), -4, "tgn: workspace too small")
    for hole in (("ids", 1), ("nbr_dt", 1), ("nbr_eid", 2)):
        _expect(lib, lvl(_weights(L), gru, _levels(L, hole), need), -1, f"tgat: null level array (level {hole[1]})")


@cpu_only
def test_tgat_training_validates_before_any_hip_call(lib):
    L, B, D = 2, 3, DUMMY
    cfg = _capi.TgatConfig(16, 16, 16, L, 2, 4)
    csr = _capi.Csr(10, 10, D, D, D, D)
    need = lib.dygnn_tgat_train_workspace_bytes(C.byref(cfg), B)
    fwd = lambda w, lv, nbytes: lib.dygnn_tgat_train_forward(C.byref(cfg), C.byref(w), C.byref(csr), lv, D, D, D, D, D, B, 0.1, 7, D, D, D, nbytes, None)
    _expect(lib, fwd(_weights(L, (1, "fc1_w")), None, need), -1, "tgat_train_forward: null layer weights (layer 1)")
    _expect(lib, fwd(_weights(L), None, need - 1), -4, "tgat_train_forward: workspace too small")
    for hole in (("ids", 1), ("nbr_eid", 1), ("nbr_dt", 2)):
        _expect(lib, fwd(_weights(L), C.byref(_levels(L, hole)), need), -1, f"tgat_train_forward: null level array (level {hole[1]})")
    bwd = lambda w, g, nbytes: lib.dygnn_tgat_backward(C.byref(cfg), C.byref(w), C.byref(g), D, D, B, 0.1, 7, D, nbytes, None)
    _expect(lib, bwd(_weights(L), _weights(L, (1, "value_w")), need), -1, "tgat_backward: null gradient buffer (layer 1)")
    _expect(lib, bwd(_weights(L, (0, "fc2_w")), _weights(L), need), -1, "tgat_backward: null layer weights (layer 0)")
    _expect(lib, bwd(_weights(L), _weights(L), need - 1), -4, "tgat_backward: workspace too small")
