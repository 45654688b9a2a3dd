"""Constant input channels of layer 0 (DYGNN_TABLE_CONST_QKV, include/dygnn.h): with the node table flagged all zero the first 48
rows of layer 0's LayerNorm output depend on the token through (mean, rstd) alone, and layer 0's Q/K/V products replace their 3 k-chunks
(6 with a zero edge table as well) by one rank-3 MFMA per output tile.  The sums are taken in another order, so the form is held to the
reference fixtures and the oracle at the project's bars (tests/parity.py), and WITHIN the form every row must keep its bits whatever kernel
shape, workgroup slot, partner, group, packing or epilogue computes it (torch.equal).  A model with impl = 0 takes the form unless its
`const_qkv` attribute is cleared, and DYGNN_CONST_QKV = 0 / 1 (read per call) forces either form.

The four-wave and the eight-wave kernels are compared as tests/test_dygformer_large_batch_gpu.py compares them — one call of 257 pairs
against calls of 128 and 129 — because DYGNN_SMALL_BATCH_KERNELS is read once per process."""
import ctypes as C

import numpy as np
import pytest
import torch

from dyglib_amd import _capi
from dyglib_amd import synthetic as syn
from oracle import dygformer_oracle as orc
from tests import golden_cases as gc
from tests.parity import close, close_scaled
from tests.test_dygformer_gpu import build_model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NODE, EDGE, CONST = _capi.TABLE_NODE_ZERO, _capi.TABLE_EDGE_ZERO, _capi.TABLE_CONST_QKV


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for name in ("DYGNN_CONST_QKV", "DYGNN_POOLED_TAIL", "DYGNN_PACK_PAIRS", "DYGNN_PROJ_TABLES"):
        monkeypatch.delenv(name, raising=False)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _call(model, *args, **kw):
    with torch.no_grad():
        out = model.compute_src_dst_node_temporal_embeddings(*args, **kw)
    torch.cuda.synchronize()
    return out


# ---- graphs and models as tests/test_dygformer_zero_tables_gpu.py builds them: 60 + 20 nodes, 3,000 edges
def _graph(edge_kind="normal", node_random=False):
    data, nf, ef = syn.make_bipartite_graph(60, 20, 3000, seed=31, edge_feat_kind=edge_kind)      # zero node table, as every reference dataset
    if node_random:
        nf[1:] = np.random.RandomState(3).standard_normal(nf[1:].shape).astype(np.float32) * 0.3
    return data, nf, ef


@pytest.fixture(scope="module")
def graphs():
    return {"node0": _graph(), "both0": _graph("zeros"), "edge0": _graph("zeros", node_random=True)}


_MODELS = {}


def _new_model(graph, params, L, P):
    from dyglib_amd import DyGFormer, get_neighbor_sampler
    data, nf, ef = graph
    sampler = get_neighbor_sampler(data, "recent", seed=1, device=DEV)
    m = DyGFormer(nf, ef, sampler, 100, 50, patch_size=P, num_layers=2, num_heads=2, dropout=0.1, max_input_sequence_length=L, device=DEV)
    m.load_state_dict({k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for k, v in params.items()})
    return m.to(DEV).eval()


def _model(graphs, which, L, P):
    key = (which, L, P)
    if key not in _MODELS:
        params = syn.make_dygformer_params(11, patch_size=P)
        _MODELS[key] = (_new_model(graphs[which], params, L, P), params)
    m, params = _MODELS[key]
    assert m.impl == 0
    return m, params


def _last(data, B):
    idx = np.arange(data.num_interactions - B, data.num_interactions)
    return data.src_node_ids[idx], data.dst_node_ids[idx], data.node_interact_times[idx]


def _capi_forward(model, src, dst, t, flags, entry="projected", impl=0):
    """one call through the C ABI with the TEST's flags (no projected tables)"""
    dev = model._device()
    s, d, tm = (model._to_dev(x, ty, dev) for x, ty in ((src, torch.int64), (dst, torch.int64), (t, torch.float64)))
    B = s.numel()
    weights, packed = model._packed_weights(dev)
    ws = model._workspace_for(B, dev)
    out_src = torch.empty((B, model.node_feat_dim), dtype=torch.float32, device=dev)
    out_dst = torch.empty_like(out_src)
    args = [C.byref(model._cfg), C.byref(weights), packed.data_ptr(), model.neighbor_sampler.csr.on_device(dev),
            model.node_raw_features.data_ptr(), model.edge_raw_features.data_ptr(), s.data_ptr(), d.data_ptr(), tm.data_ptr(), B, 0, 0,
            out_src.data_ptr(), out_dst.data_ptr(), ws.data_ptr(), ws.numel(), None, impl, _capi.current_stream_ptr(), flags]
    if entry == "projected":
        rc = model._lib.dygnn_dygformer_forward_projected(*args, None, None)
    else:
        rc = model._lib.dygnn_dygformer_forward_tables(*args)
    _capi.check(rc)
    torch.cuda.synchronize()
    return out_src, out_dst


# ---- the reference fixtures --------------------------------------------------------------------
# the headline P = 2 / L = 64; P = 4 with a source window of 8 = padded lengths (8, 48); the 128-token kernel
@pytest.mark.parametrize("name", ["bip_p2_l64", "hub_p4_l48", "bip_p8_l512"])
def test_short_form_against_the_reference_fixtures(name, monkeypatch):
    c, g = gc.build_case(name), gc.load_golden(name)
    model, _ = build_model(c)
    assert model.impl == 0 and model.table_flags == NODE and model._const_qkv_flag() == CONST
    P = c["cfg"]["patch_size"]
    T = (g["src_pad_ids"].shape[1] + g["dst_pad_ids"].shape[1]) // P
    R = gc.TAP_ROWS
    out = {}
    for form in ("1", "0", None):           # forced on, forced off, the class's own bit (= on)
        if form is None:
            monkeypatch.delenv("DYGNN_CONST_QKV")
        else:
            monkeypatch.setenv("DYGNN_CONST_QKV", form)
        taps = {}
        se, de = _call(model, c["src"], c["dst"], c["times"], _taps=taps)
        nse, nde = _call(model, c["src"], c["neg_dst"], c["times"])
        close_scaled(taps["encoder_input"][:R, :T].cpu().numpy(), g["encoder_input_rows"], f"{name} const-qkv {form} encoder input")
        for l in range(2):
            close_scaled(taps["layer_outputs"][l][:R, :T].cpu().numpy(), g[f"layer{l}_rows"], f"{name} const-qkv {form} layer {l} (internal tap, scaled bar)")
        close(se.cpu().numpy(), g["src_emb"], f"{name} const-qkv {form} src emb")
        close(de.cpu().numpy(), g["dst_emb"], f"{name} const-qkv {form} dst emb")
        close(nse.cpu().numpy(), g["neg_src_emb"], f"{name} const-qkv {form} neg src emb")
        close(nde.cpu().numpy(), g["neg_dst_emb"], f"{name} const-qkv {form} neg dst emb")
        out[form] = (taps["encoder_input"], taps["layer_outputs"][0], se, de)
    assert torch.equal(out["1"][0], out["0"][0])                 # the encoder input is the same computation
    d0 = float((out["1"][1] - out["0"][1]).abs().max())
    print(f"{name}: largest difference between the forms: layer 0 output {d0:.3e}, src emb {float((out['1'][2] - out['0'][2]).abs().max()):.3e}")
    assert not torch.equal(out["1"][1], out["0"][1])             # the short path did run: another order of summation
    assert all(torch.equal(a, b) for a, b in zip(out[None], out["1"]))      # the class sets the bit itself
    model.const_qkv = False                                                 # ... unless told not to
    assert _same(_call(model, c["src"], c["dst"], c["times"]), out["0"][2:])


def test_nonzero_node_table_keeps_the_full_product(monkeypatch):
    name = "gen_p1_l32"
    c, g = gc.build_case(name), gc.load_golden(name)
    model, _ = build_model(c)
    assert model.table_flags == 0 and model.const_qkv and model._const_qkv_flag() == 0
    out = {}
    for form in ("1", "0"):
        monkeypatch.setenv("DYGNN_CONST_QKV", form)
        taps = {}
        se, de = _call(model, c["src"], c["dst"], c["times"], _taps=taps)
        close(se.cpu().numpy(), g["src_emb"], f"{name} const-qkv {form} src emb")
        out[form] = (taps["layer_outputs"][0], taps["layer_outputs"][1], se, de)
    assert all(torch.equal(a, b) for a, b in zip(out["1"], out["0"]))


# ---- torch.equal within the form, L = 64 / P = 2 ------------------------------------------------
def test_rows_do_not_depend_on_kernel_family_packing_or_epilogue(graphs, monkeypatch):
    """257 pairs in the eight-wave kernel (the last workgroup half full) against 128 + 129 in the four-wave kernel; the packed kernel;
    the deferred tail"""
    model, _ = _model(graphs, "node0", 64, 2)
    src, dst, t = _last(graphs["node0"][0], 257)
    big = _call(model, src, dst, t)
    lo, hi = _call(model, src[:128], dst[:128], t[:128]), _call(model, src[128:], dst[128:], t[128:])
    assert torch.equal(big[0], torch.cat([lo[0], hi[0]])) and torch.equal(big[1], torch.cat([lo[1], hi[1]]))
    monkeypatch.setenv("DYGNN_PACK_PAIRS", "1")                  # the packed kernel (and its deferred tail)
    assert _same(_call(model, src, dst, t), big)
    monkeypatch.setenv("DYGNN_PACK_PAIRS", "0")
    assert _same(_call(model, src, dst, t), big)
    monkeypatch.setenv("DYGNN_POOLED_TAIL", "1")                 # the unpacked kernels that end with the token means
    assert _same(_call(model, src, dst, t), big) and _same(_call(model, src[:128], dst[:128], t[:128]), lo)
    monkeypatch.setenv("DYGNN_POOLED_TAIL", "0")
    assert _same(_call(model, src, dst, t), big)
    monkeypatch.setenv("DYGNN_CONST_QKV", "0")
    assert not _same(_call(model, src, dst, t), big)             # the full product is another sum


def test_tapped_against_untapped(graphs):
    model, _ = _model(graphs, "node0", 64, 2)
    src, dst, t = _last(graphs["node0"][0], 9)
    taps = {}
    assert _same(_call(model, src, dst, t, _taps=taps), _call(model, src, dst, t))
    assert float(taps["layer_outputs"][-1].abs().max()) > 0


def _three_calls(data, B):
    """three calls of B pairs with different padded lengths: the first interactions (empty and short histories: 10 tokens), early ones
    (44 tokens: the third token tile partly empty), and the last ones (full windows: 64 tokens)"""
    n = data.num_interactions
    idx = np.stack([np.arange(B), np.arange(150, 150 + B), np.arange(n - B, n)])
    return data.src_node_ids[idx], data.dst_node_ids[idx], data.node_interact_times[idx]


def test_groups_of_different_padded_lengths(graphs):
    """three calls of 43 pairs in one launch — a workgroup holds the last pair of one call and the first of the next — against the calls alone"""
    model, _ = _model(graphs, "node0", 64, 2)
    src, dst, t = _three_calls(graphs["node0"][0], 43)
    with torch.no_grad():
        s, d = model.compute_src_dst_node_temporal_embeddings_many(src, dst, t)
    lens = []
    for i in range(3):
        taps = {}
        a, b = _call(model, src[i], dst[i], t[i], _taps=taps)
        lens.append(tuple(taps["seq_lens"].cpu().tolist()))
        assert torch.equal(s[i], a) and torch.equal(d[i], b), i
    assert len(set(lens)) == 3, lens


def test_positive_and_negative_halves_against_separate_calls(graphs):
    model, _ = _model(graphs, "node0", 64, 2)
    data = graphs["node0"][0]
    n = 40
    src, dst, t = _last(data, n)
    neg = syn.random_negative_dst(np.random.RandomState(4), np.unique(data.dst_node_ids), n)
    nsrc = src.copy()
    nsrc[5] = next(v for v in src if v != src[5])            # a "negative" with another source: the plain path inside the pairing
    with torch.no_grad():
        s, d = model.compute_src_dst_node_temporal_embeddings_many(np.stack([src, nsrc]), np.stack([dst, neg]), np.stack([t, t]), pos_neg_halves=True)
    pos, ngv = _call(model, src, dst, t), _call(model, nsrc, neg, t)
    assert torch.equal(s[0], pos[0]) and torch.equal(d[0], pos[1])
    assert torch.equal(s[1], ngv[0]) and torch.equal(d[1], ngv[1])


def test_empty_histories_and_a_half_empty_last_tile(graphs, monkeypatch):
    """the first 40 interactions: nodes seen for the first time (empty histories) and windows of a few neighbours, so the padded call is
    short and its last token tile partly empty; every kernel form gives the same bits, and they are the oracle's"""
    model, params = _model(graphs, "node0", 64, 2)
    data, nf, ef = graphs["node0"]
    src, dst, t = data.src_node_ids[:40], data.dst_node_ids[:40], data.node_interact_times[:40]
    assert len(np.unique(src)) + len(np.unique(dst)) > 2      # several first appearances = empty histories
    taps = {}
    tapped = _call(model, src, dst, t, _taps=taps)
    S_s, S_d = taps["seq_lens"].cpu().tolist()
    T = (S_s + S_d) // 2
    assert T % 16 != 0, (S_s, S_d)
    plain = _call(model, src, dst, t)
    assert _same(tapped, plain)
    monkeypatch.setenv("DYGNN_PACK_PAIRS", "1")
    assert _same(_call(model, src, dst, t), plain)
    monkeypatch.setenv("DYGNN_PACK_PAIRS", "0")
    monkeypatch.setenv("DYGNN_POOLED_TAIL", "1")
    assert _same(_call(model, src, dst, t), plain)
    adj = orc.OracleAdjacency(data.src_node_ids, data.dst_node_ids, data.edge_ids, data.node_interact_times)
    with torch.no_grad():
        os_, od = orc.dygformer_forward(params, nf, ef, adj, src, dst, t, 2, 64)
    close(plain[0].cpu().numpy(), os_.numpy(), "const-qkv, first interactions: src emb")
    close(plain[1].cpu().numpy(), od.numpy(), "const-qkv, first interactions: dst emb")


# ---- both tables zero: the 96-row prefix ---------------------------------------------------------
@pytest.mark.parametrize("L,P,B", [(64, 2, 24), (512, 8, 3)])
def test_both_tables_zero_against_the_oracle(graphs, L, P, B, monkeypatch):
    model, params = _model(graphs, "both0", L, P)
    assert model.table_flags == NODE | EDGE
    data, nf, ef = graphs["both0"]
    src, dst, t = _last(data, B)
    adj = orc.OracleAdjacency(data.src_node_ids, data.dst_node_ids, data.edge_ids, data.node_interact_times)
    with torch.no_grad():
        os_, od = orc.dygformer_forward(params, nf, ef, adj, src, dst, t, P, L)
    got = _call(model, src, dst, t)
    close(got[0].cpu().numpy(), os_.numpy(), f"const-qkv, both tables zero L={L}: src emb")
    close(got[1].cpu().numpy(), od.numpy(), f"const-qkv, both tables zero L={L}: dst emb")
    assert _same(_capi_forward(model, src, dst, t, NODE | EDGE | CONST), got)
    short3 = _capi_forward(model, src, dst, t, NODE | CONST)                # the node prefix alone (the edge table unflagged): 3 chunks, another sum
    close(short3[0].cpu().numpy(), os_.numpy(), f"const-qkv, node prefix of two zero tables L={L}: src emb")
    assert not _same(short3, got)
    monkeypatch.setenv("DYGNN_CONST_QKV", "0")
    full = _call(model, src, dst, t)
    assert not _same(full, got) and not _same(full, short3)
    assert _same(full, _capi_forward(model, src, dst, t, NODE | EDGE, entry="tables"))


@pytest.mark.parametrize("L,P,B", [(64, 2, 24), (512, 8, 3)])
def test_zero_edge_table_with_a_random_node_table_is_no_prefix(graphs, L, P, B):
    model, _ = _model(graphs, "edge0", L, P)
    assert model.table_flags == EDGE
    src, dst, t = _last(graphs["edge0"][0], B)
    plain = _capi_forward(model, src, dst, t, EDGE)
    assert _same(_capi_forward(model, src, dst, t, EDGE | CONST), plain)
    assert _same(_capi_forward(model, src, dst, t, CONST), _capi_forward(model, src, dst, t, 0))


# ---- the constants follow the weights ------------------------------------------------------------
def test_constants_are_refreshed_after_a_weight_update(graphs):
    params = syn.make_dygformer_params(11, patch_size=2)
    model = _new_model(graphs["node0"], params, 64, 2)
    src, dst, t = _last(graphs["node0"][0], 24)
    before = _call(model, src, dst, t)                      # the kernel-ready copy exists: the update below is an in-place repack
    tr = model.transformers[0]
    stepped = [tr.norm_layers[0].weight, tr.norm_layers[0].bias, tr.multi_head_attention.in_proj_weight, model.projection_layer["node"].bias]
    gen = torch.Generator(device="cpu").manual_seed(7)
    for p in stepped:
        p.grad = (torch.randn(p.shape, generator=gen) * 0.5).to(p.device)
    torch.optim.SGD(stepped, lr=0.1).step()
    after = _call(model, src, dst, t)
    assert not _same(after, before)
    fresh = _new_model(graphs["node0"], {k: v.detach().cpu() for k, v in model.state_dict().items()}, 64, 2)
    assert _same(_call(fresh, src, dst, t), after)


# ---- the bit's scope -------------------------------------------------------------------------------
def test_the_bit_belongs_to_forward_projected_alone(graphs):
    model, _ = _model(graphs, "node0", 64, 2)
    src, dst, t = _last(graphs["node0"][0], 5)
    with pytest.raises(Exception):
        _capi_forward(model, src, dst, t, NODE | CONST, entry="tables")
    with pytest.raises(Exception):
        _capi_forward(model, src, dst, t, 64)
    plain = _capi_forward(model, src, dst, t, NODE, entry="tables")
    assert _same(_capi_forward(model, src, dst, t, NODE), plain)                  # forward_projected without the bit IS forward_tables
    assert _same(_capi_forward(model, src, dst, t, NODE, impl=3), plain)
    assert not _same(_capi_forward(model, src, dst, t, NODE | CONST), plain)
    model.impl = 3                                                                # impl = 3 names the full product: the class leaves the bit out
    try:
        assert _same(_call(model, src, dst, t), plain)
    finally:
        model.impl = 0
