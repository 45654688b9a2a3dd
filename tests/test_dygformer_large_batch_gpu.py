"""Inference above 256 pairs: k_dygformer_fused3<4, false, 8, 1> (untapped) and <4, false, 8, 2> (tapped), two pairs per eight-wave
workgroup, (B + 1) / 2 workgroups — at ODD call sizes and an ODD group size, which the suite's other large launches (4 x 80 pairs) do not have.

Recipes: tests/large_batch_cases.py.  With B odd the very last row of a call is the lone pair of a half-full workgroup: its partner slot
must neither read nor write anything, and the row must come out as it does from a four-wave workgroup of its own
(test_rows_do_not_depend_on_kernel_family compares exactly that row, among the others, bit for bit).  With a group size of 87 one workgroup
of the grouped launch holds the last pair of one call and the first pair of the next, each padded to its own call's lengths.
Every test forces the fused path (impl = 3) and runs under torch.no_grad().  Bars: tests/parity.py, embeddings plain 1e-4, the per-token
taps 1e-4 * max(1, max|reference|), against the CPU oracle."""
import re

import numpy as np
import pytest
import torch

from oracle import dygformer_oracle as orc
from tests import large_batch_cases as lb
from tests.parity import close, close_scaled
from tests.test_dygformer_gpu import build_model

pytestmark = pytest.mark.gpu


def _oracle(c, src, dst, times, taps=None):
    d, cfg = c["data"], c["cfg"]
    adj = orc.OracleAdjacency(d.src_node_ids, d.dst_node_ids, d.edge_ids, d.node_interact_times)
    with torch.no_grad():
        s, t = orc.dygformer_forward(c["params"], c["node_feat"], c["edge_feat"], adj, src, dst, times, cfg["patch_size"],
                                     cfg["max_input_sequence_length"], cfg["num_heads"], cfg["num_layers"], taps=taps)
    return s.numpy(), t.numpy()


@pytest.mark.parametrize("name,B", [("full64", 257), ("full64", 401), ("ragged40", 411), ("hub14", 257)])
def test_odd_batches_against_oracle(name, B):
    c = lb.build(name, B)
    assert len(c["src"]) == B and B % 2 == 1
    model, _ = build_model(c)
    model.impl = 3
    otaps, taps = {}, {}
    ws, wd = _oracle(c, c["src"], c["dst"], c["times"], otaps)
    with torch.no_grad():
        s, d = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"])
        ts, td = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], _taps=taps)
    tag = f"{name}-{B}"
    close(s.cpu().numpy(), ws, f"{tag} src emb", label=f"eight-wave inference vs oracle, {tag}, src emb")
    close(d.cpu().numpy(), wd, f"{tag} dst emb", label=f"eight-wave inference vs oracle, {tag}, dst emb")
    assert torch.equal(ts, s) and torch.equal(td, d)          # the tapped instance streams the full last layer; its embeddings are the pooled ones
    (S_s, S_d), = c["seq_lens"]
    assert tuple(taps["seq_lens"].cpu().tolist()) == (S_s, S_d)
    T = (S_s + S_d) // c["cfg"]["patch_size"]
    assert otaps["encoder_input"].shape[1] == T and len(otaps["layer_outputs"]) == c["cfg"]["num_layers"]
    for l, ref in enumerate(otaps["layer_outputs"]):
        got = taps["layer_outputs"][l]
        close_scaled(got[:, :T].cpu().numpy(), ref.numpy(), f"{tag} layer {l} rows",
                     label=f"eight-wave inference vs oracle, {tag}, tapped rows of layer {l}")
        assert not bool(got[:, T:].any())                     # no pair wrote past its T tokens


def test_rows_do_not_depend_on_kernel_family():
    """One call of 257 pairs (eight-wave, two pairs per workgroup) against the same rows as calls of 128 and 129 pairs (four-wave, one pair per
    workgroup).  All three pad to the same lengths — asserted through the taps — so every row must agree bit for bit, row 256 (alone in
    workgroup 128 of the large call) included."""
    c = lb.build("full64")
    model, _ = build_model(c)
    model.impl = 3
    src, dst, t = c["src"], c["dst"], c["times"]
    parts = [slice(0, 257), slice(0, 128), slice(128, 257)]
    plain, tapped, lens = [], [], []
    with torch.no_grad():
        for sl in parts:
            taps = {}
            plain.append(model.compute_src_dst_node_temporal_embeddings(src[sl], dst[sl], t[sl]))
            tapped.append(model.compute_src_dst_node_temporal_embeddings(src[sl], dst[sl], t[sl], _taps=taps) + (taps["layer_outputs"],))
            lens.append(tuple(taps["seq_lens"].cpu().tolist()))
    assert lens == [(64, 64)] * 3, lens
    for side in (0, 1):
        whole = plain[0][side]
        assert torch.equal(whole[:128], plain[1][side]) and torch.equal(whole[128:], plain[2][side]), side
        assert torch.equal(whole[256], plain[2][side][128])                                       # the lone pair of the half-full workgroup
        assert torch.equal(tapped[0][side][:128], tapped[1][side]) and torch.equal(tapped[0][side][128:], tapped[2][side]), side
    for l in range(c["cfg"]["num_layers"]):                                                       # ... and so must every token row of every layer
        assert torch.equal(tapped[0][2][l][:128], tapped[1][2][l]) and torch.equal(tapped[0][2][l][128:], tapped[2][2][l]), l


def test_group_boundary_inside_a_workgroup():
    c = lb.build("hub_groups")
    model, _ = build_model(c)
    model.impl = 3
    src, dst, t = c["src"], c["dst"], c["times"]
    assert src.shape == (3, 87)
    with torch.no_grad():
        ms, md = model.compute_src_dst_node_temporal_embeddings_many(src, dst, t, pos_neg_halves=False)
        assert ms.shape == md.shape == (3, 87, 172)
        lens = []
        for i in range(3):
            taps = {}
            s1, d1 = model.compute_src_dst_node_temporal_embeddings(src[i], dst[i], t[i])
            model.compute_src_dst_node_temporal_embeddings(src[i], dst[i], t[i], _taps=taps)
            lens.append(tuple(taps["seq_lens"].cpu().tolist()))
            assert torch.equal(ms[i], s1) and torch.equal(md[i], d1), i          # every call keeps its own padded lengths, also inside workgroup 43
            ws, wd = _oracle(c, src[i], dst[i], t[i])
            close(ms[i].cpu().numpy(), ws, f"hub_groups call {i} src emb", label=f"grouped eight-wave launch, odd group size, vs oracle, call {i} src emb")
            close(md[i].cpu().numpy(), wd, f"hub_groups call {i} dst emb", label=f"grouped eight-wave launch, odd group size, vs oracle, call {i} dst emb")
    assert lens == c["seq_lens"] and len(set(lens)) == 3, lens


# ---- which kernels ran ------------------------------------------------------------------------------------------------------------
_KERNELS = ("k_dygformer_fused3", "k_attn_bwd", "k_ffn_bwd")


def _instance(name: str):
    """('k_ffn_bwd', (8,)) from either spelling of a kernel name: demangled `... k_ffn_bwd<8>(...)`, or mangled `..9k_ffn_bwdILi8EE...`;
    booleans as 0 / 1.  None for any other kernel."""
    for k in _KERNELS:
        m = re.search(k + r"<([^>]*)>", name)
        if m:
            args = [re.sub(r"\([^)]*\)", "", a).strip() for a in m.group(1).split(",")]
            return k, tuple({"true": 1, "false": 0}.get(a, int(a) if a.lstrip("-").isdigit() else a) for a in args)
        m = re.search(k + r"I((?:L[a-z]\d+E)+)E", name)
        if m:
            return k, tuple(int(v) for v in re.findall(r"L[a-z](\d+)E", m.group(1)))
    return None


def test_large_calls_really_take_the_eight_wave_kernels():
    """The parity tests above choose their kernels by call size alone; this one reads the recorded kernel names to confirm that the sizes do
    select the eight-wave instances (template arguments: k_dygformer_fused3<TPW, TR, NW, PL>, k_attn_bwd<TPW, NW = 8>, k_ffn_bwd<NW>)."""
    from torch.profiler import ProfilerActivity, profile
    c = lb.build("full64")
    model, _ = build_model(c)
    model.impl = 3
    G = torch.ones((257, 172), device="cuda:0")

    def step():
        with torch.no_grad():
            model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"])
        for p in model.parameters():
            p.grad = None
        s, d = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"])          # eval mode, autograd on: the training kernels
        ((s * G).sum() + (d * G).sum()).backward()
        torch.cuda.synchronize()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        step()                                                   # packing and first-use work stay out of the trace
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    if not names:
        pytest.skip("this torch build's profiler recorded no device kernels")
    seen = {i for i in map(_instance, names) if i is not None}
    assert seen, sorted(set(names))[:40]
    fused = {a for k, a in seen if k == "k_dygformer_fused3"}
    attn = {a + (8,) * (2 - len(a)) for k, a in seen if k == "k_attn_bwd"}          # NW defaults to 8; a demangler may leave a default out
    ffn = {a for k, a in seen if k == "k_ffn_bwd"}
    assert {a[:3] for a in fused} == {(4, 1, 8), (4, 0, 8)}, fused                   # training and inference forward: eight waves, none with four
    assert attn == {(4, 8)}, attn
    assert ffn == {(8,)}, ffn
