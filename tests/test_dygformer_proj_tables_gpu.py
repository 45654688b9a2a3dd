"""Projected feature tables of the fused DyGFormer inference path (dygformer_proj_tables.hip): W[:, slot p] . table[row] is
computed once per (row, patch slot) and weights version, and the kernel adds P gathered rows per token instead of running the node / edge
product.  The sum is split per slot, so the two forms differ in the last bits: both are held to the reference fixtures at the project's bars
(tests/parity.py), and WITHIN the projected form every row must keep its bits whatever kernel shape, workgroup slot, partner, group or
epilogue computes it (torch.equal).  DYGNN_PROJ_TABLES = 0 / 1 (read per call) puts a model with impl = 0 on either form.

The four-wave and the eight-wave kernels are compared as tests/test_dygformer_large_batch_gpu.py compares them — one call of 257 pairs
against calls of 128 and 129 — because DYGNN_SMALL_BATCH_KERNELS is read once per process."""
import numpy as np
import pytest
import torch

from dyglib_amd import _capi
from dyglib_amd import synthetic as syn
from oracle import dygformer_oracle as orc
from tests import golden_cases as gc
from tests import large_batch_cases as lb
from tests.parity import close, close_scaled
from tests.test_dygformer_gpu import build_model

pytestmark = pytest.mark.gpu


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _call(model, *args, **kw):
    with torch.no_grad():
        out = model.compute_src_dst_node_temporal_embeddings(*args, **kw)
    torch.cuda.synchronize()
    return out


def _uses_tables(model, want):
    """the projected tables this model's last inference call was given"""
    assert model._tables.built == set(want), model._tables.built


@pytest.fixture(autouse=True)
def projected(monkeypatch):
    monkeypatch.setenv("DYGNN_PROJ_TABLES", "1")
    monkeypatch.delenv("DYGNN_POOLED_TAIL", raising=False)


# P = 1 (and a non-zero node table); the headline P = 2 / L = 64; P = 4 with a source window of 8 = padded lengths (8, 48); the 128-token kernel
@pytest.mark.parametrize("name", ["gen_p1_l32", "bip_p2_l64", "hub_p4_l48", "bip_p8_l512"])
def test_both_forms_against_the_reference_fixtures(name, monkeypatch):
    c, g = gc.build_case(name), gc.load_golden(name)
    model, _ = build_model(c)
    assert model.impl == 0
    P = c["cfg"]["patch_size"]
    T = (g["src_pad_ids"].shape[1] + g["dst_pad_ids"].shape[1]) // P
    out = {}
    for form in ("0", "1"):
        monkeypatch.setenv("DYGNN_PROJ_TABLES", form)
        taps = {}
        se, de = _call(model, c["src"], c["dst"], c["times"], _taps=taps)
        nse, nde = _call(model, c["src"], c["neg_dst"], c["times"])
        enc = taps["encoder_input"][:gc.TAP_ROWS, :T]
        close_scaled(enc.cpu().numpy(), g["encoder_input_rows"], f"{name} form {form} encoder input")
        close(se.cpu().numpy(), g["src_emb"], f"{name} form {form} src emb")
        close(de.cpu().numpy(), g["dst_emb"], f"{name} form {form} dst emb")
        close(nse.cpu().numpy(), g["neg_src_emb"], f"{name} form {form} neg src emb")
        close(nde.cpu().numpy(), g["neg_dst_emb"], f"{name} form {form} neg dst emb")
        out[form] = (enc, se, de)
    _uses_tables(model, {"edge"} | ({"node"} if c["node_feat"].any() else set()))
    diffs = [float((a - b).abs().max()) for a, b in zip(out["0"], out["1"])]
    print(f"{name}: largest difference between the forms: encoder input {diffs[0]:.3e}, src emb {diffs[1]:.3e}, dst emb {diffs[2]:.3e}")
    assert diffs[0] > 0          # the projected form did run: the split sum rounds differently somewhere in 3 x T x 200 elements


@pytest.fixture(scope="module")
def full64():
    c = lb.build("full64")           # P = 2, L = 64, 257 pairs, non-zero node AND edge table
    model, _ = build_model(c)
    return c, model


@pytest.fixture(scope="module")
def ragged40():
    c = lb.build("ragged40", 43)     # P = 2, L = 40: 20 source tokens (not a multiple of 16), T = 40 (the last tile half empty); 3 empty histories
    model, _ = build_model(c)
    return c, model


def test_rows_do_not_depend_on_kernel_family_or_epilogue(full64, monkeypatch):
    """257 pairs in the eight-wave kernel (the last workgroup half full) against 128 + 129 in the four-wave kernel; then both epilogues"""
    c, model = full64
    src, dst, t = c["src"], c["dst"], c["times"]
    big = _call(model, src, dst, t)
    _uses_tables(model, {"node", "edge"})
    lo, hi = _call(model, src[:128], dst[:128], t[:128]), _call(model, src[128:], dst[128:], t[128:])
    assert torch.equal(big[0], torch.cat([lo[0], hi[0]])) and torch.equal(big[1], torch.cat([lo[1], hi[1]]))
    monkeypatch.setenv("DYGNN_POOLED_TAIL", "1")
    assert _same(_call(model, src, dst, t), big) and _same(_call(model, src[:128], dst[:128], t[:128]), lo)
    monkeypatch.setenv("DYGNN_POOLED_TAIL", "0")
    assert _same(_call(model, src, dst, t), big)
    monkeypatch.setenv("DYGNN_PROJ_TABLES", "0")
    assert not _same(_call(model, src, dst, t), big)          # the MFMA form is another sum


def test_tapped_against_untapped(full64):
    c, model = full64
    src, dst, t = c["src"][-9:], c["dst"][-9:], c["times"][-9:]
    taps = {}
    assert _same(_call(model, src, dst, t, _taps=taps), _call(model, src, dst, t))
    assert float(taps["layer_outputs"][-1].abs().max()) > 0


def test_groups_of_different_padded_lengths():
    """three calls of 87 pairs of the hub graph in one launch — a workgroup holds the last pair of one call and the first of the next —
    against the three calls alone"""
    c = lb.build("hub_groups")
    model, _ = build_model(c)
    with torch.no_grad():
        s, d = model.compute_src_dst_node_temporal_embeddings_many(c["src"], c["dst"], c["times"])
    lens = []
    for i in range(3):
        taps = {}
        a, b = _call(model, c["src"][i], c["dst"][i], c["times"][i], _taps=taps)
        lens.append(tuple(taps["seq_lens"].cpu().tolist()))
        assert torch.equal(s[i], a) and torch.equal(d[i], b), i
    assert lens == c["seq_lens"]
    _uses_tables(model, {"edge"})


def test_positive_and_negative_halves_against_separate_calls(ragged40):
    """[2, 40] with pos_neg_halves: the second pair of a workgroup copies the first pair's source rows where source and time agree (only the
    first source tile is whole: 20 source tokens) and projects its own where they do not"""
    c, model = ragged40
    data = c["data"]
    n = 40
    src, dst, t = c["src"][-n:], c["dst"][-n:], c["times"][-n:]
    neg = syn.random_negative_dst(np.random.RandomState(4), np.unique(data.dst_node_ids), n)
    nsrc, nt = src.copy(), t.copy()
    for i in (5, 17):                                   # a "negative" with another source
        nsrc[i] = next(v for v in src if v != src[i])
    nt[9] = t[9] - 1000.0                               # ... and one at another time
    with torch.no_grad():
        s, d = model.compute_src_dst_node_temporal_embeddings_many(np.stack([src, nsrc]), np.stack([dst, neg]), np.stack([t, nt]), pos_neg_halves=True)
    _uses_tables(model, {"node", "edge"})
    taps = {}
    pos, ngt = _call(model, src, dst, t, _taps=taps), _call(model, nsrc, neg, nt)
    assert taps["seq_lens"].cpu().tolist()[0] // 2 % 16 != 0
    assert torch.equal(s[0], pos[0]) and torch.equal(d[0], pos[1])
    assert torch.equal(s[1], ngt[0]) and torch.equal(d[1], ngt[1])


def test_empty_histories_a_half_empty_tile_and_both_tables_against_the_oracle(ragged40):
    """3 first interactions (no history: every position but the query's own is absent) + 40 late ones, T = 40 tokens in three tiles, non-zero
    node and edge tables; and the 3 alone, where T = 2"""
    c, model = ragged40
    d = c["data"]
    adj = orc.OracleAdjacency(d.src_node_ids, d.dst_node_ids, d.edge_ids, d.node_interact_times)
    for tag, sl in (("43 pairs", slice(None)), ("3 pairs without history", slice(0, 3))):
        src, dst, t = c["src"][sl], c["dst"][sl], c["times"][sl]
        gs, gd = _call(model, src, dst, t)
        with torch.no_grad():
            os_, od = orc.dygformer_forward(c["params"], c["node_feat"], c["edge_feat"], adj, src, dst, t, 2, 40)
        close(gs.cpu().numpy(), os_.numpy(), f"projected tables, {tag}: src emb")
        close(gd.cpu().numpy(), od.numpy(), f"projected tables, {tag}: dst emb")
    _uses_tables(model, {"node", "edge"})


def test_all_zero_edge_table_unflagged_gives_the_bits_of_the_flagged_call():
    from dyglib_amd import DyGFormer, get_neighbor_sampler
    data, nf, ef = syn.make_bipartite_graph(60, 20, 3000, seed=31, edge_feat_kind="zeros")
    nf[1:] = np.random.RandomState(3).standard_normal(nf[1:].shape).astype(np.float32) * 0.3
    model = DyGFormer(nf, ef, get_neighbor_sampler(data, "recent", seed=1, device="cuda:0"), 100, 50, patch_size=2, num_layers=2, num_heads=2,
                      dropout=0.1, max_input_sequence_length=64, device="cuda:0")
    model.load_state_dict({k: torch.from_numpy(v) for k, v in syn.make_dygformer_params(11, patch_size=2).items()})
    model = model.to("cuda:0").eval()
    src, dst, t = data.src_node_ids[-70:], data.dst_node_ids[-70:], data.node_interact_times[-70:]
    assert model.table_flags == _capi.TABLE_EDGE_ZERO
    flagged = _call(model, src, dst, t)
    _uses_tables(model, {"node"})
    model._set_table("edge", model.edge_raw_features, all_zero=False)          # the same zeros, without the promise
    assert model.table_flags == 0
    assert _same(_call(model, src, dst, t), flagged)
    _uses_tables(model, {"node", "edge"})


def test_a_cap_below_the_table_size_keeps_the_mfma_path(full64, monkeypatch):
    c, model = full64
    src, dst, t = c["src"][-20:], c["dst"][-20:], c["times"][-20:]
    monkeypatch.setenv("DYGNN_PROJ_TABLES", "0")
    plain = _call(model, src, dst, t)
    monkeypatch.delenv("DYGNN_PROJ_TABLES")
    edge_bytes = model._proj_plan()["edge"]
    try:
        model.proj_table_max_bytes = edge_bytes - 1                            # the (smaller) node table still fits
        assert set(model._proj_plan()) == {"node"}
        mixed = _call(model, src, dst, t)
        model.proj_table_max_bytes = 0
        assert _same(_call(model, src, dst, t), plain)
        model.proj_table_max_bytes = 1 << 30
        both = _call(model, src, dst, t)
    finally:
        model.proj_table_max_bytes = 1 << 30
    assert not _same(mixed, plain) and not _same(mixed, both)
    for a, b in zip(mixed, plain):
        close(a.cpu().numpy(), b.cpu().numpy(), "node table projected alone vs the MFMA path")


def test_an_optimizer_step_on_the_projection_weights_rebuilds_the_tables():
    c = gc.build_case("bip_p2_l64")
    model, _ = build_model(c)
    before = _call(model, c["src"], c["dst"], c["times"])
    opt = torch.optim.SGD(model.projection_layer.parameters(), lr=0.05)
    rs = torch.Generator().manual_seed(5)
    for p in model.projection_layer.parameters():
        p.grad = torch.randn(p.shape, generator=rs).to(p.device)
    opt.step()                                                                 # in place: same addresses, new version counters
    after = _call(model, c["src"], c["dst"], c["times"])
    assert not _same(after, before)
    fresh, _ = build_model(c)
    fresh.load_state_dict(model.state_dict())
    assert _same(_call(fresh, c["src"], c["dst"], c["times"]), after)
    _uses_tables(fresh, {"edge"})
