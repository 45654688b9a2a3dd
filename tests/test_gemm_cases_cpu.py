"""Conditions on the case table of tests/gemm_cases.py and on the host-only side of dygnn_mm / dygnn_dw_grouped (no GPU): the bars of
tests/test_gemm_gpu.py only mean what they say while these hold."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import gemm_cases as gc


@pytest.fixture(scope="module")
def lib():
    from dyglib_amd import _build, _capi
    _build.build(verbose=False)          # hipcc cross-compiles gfx950 without a GPU
    return _capi.load()


def plan(lib, fields):
    from dyglib_amd import _capi
    ks, f4 = C.c_int32(-7), C.c_int32(-7)
    args = _capi.MmArgs(**fields)
    kernel = lib.dygnn_mm_plan(C.byref(args), C.byref(ks), C.byref(f4))
    assert lib.dygnn_mm_path(C.byref(args)) == kernel
    return kernel, ks.value, f4.value


def case_plan(lib, c, monkeypatch):
    if c["dma_env"] is None:
        monkeypatch.delenv("DYGNN_MM_DMA", raising=False)
    else:
        monkeypatch.setenv("DYGNN_MM_DMA", c["dma_env"])
    return plan(lib, gc.fake_fields(c))


def test_every_case_takes_the_kernel_split_and_epilogue_the_table_intends(lib, monkeypatch):
    for c in gc.MM_CASES:
        kernel, ks, f4 = case_plan(lib, c, monkeypatch)
        if c["kernel"] < 0:
            assert kernel == c["kernel"] == gc.E_UNSUPPORTED and (ks, f4) == (-7, -7), c["name"]
            assert lib.dygnn_last_error().startswith(b"mm: "), c["name"]
        else:
            assert (kernel, ks, bool(f4)) == (c["kernel"], c["ksplit"], c["f4"]), (c["name"], kernel, ks, f4)
        if not c["tA"] and c["tB"] and c["batch"] == 1 and c["kernel"] >= 0:      # what the backbones ask before they pass a row table
            f = gc.fake_fields(c)
            assert lib.dygnn_mm_gathers_rows(f["A"], c["lda"], f["B"], c["ldb"], c["M"], c["N"], c["K"]) == int(kernel == gc.DMA), c["name"]


def test_the_table_reaches_every_kernel_orientation_epilogue_split_and_colsum_route():
    run = gc.MM_RUN
    for kernel in (gc.SMALL, gc.BIG, gc.DMA):
        for tA, tB in gc.ORIENT:
            mine = [c for c in run if c["kernel"] == kernel and (c["tA"], c["tB"]) == (tA, tB)]
            assert mine, (kernel, tA, tB)
            assert any(c["ksplit"] > 1 for c in mine), ("split", kernel, tA, tB)
        assert {c["ksplit"] for c in run if c["kernel"] == kernel} >= {1, 8, 9}
        assert any(c["colsum"] and c["ksplit"] == 1 for c in run if c["kernel"] == kernel)      # ride-along (DMA, big), stand-alone (k_mm)
        assert any(c["colsum"] and c["ksplit"] > 1 for c in run if c["kernel"] == kernel)
        assert {c["m_dev"] for c in run if c["kernel"] == kernel and c["M"] == 132} >= {0, 1, 64, 65, 132}
        assert any(c["relu"] and c["bias"] for c in run if c["kernel"] == kernel)
        assert any(c["batch"] == 6 and c["H"] == 3 for c in run if c["kernel"] == kernel)
        # all six strides at once, non-zero and pairwise different: two of them swapped in a call cannot go unseen
        assert any(c["batch"] == 4 and c["H"] == 2 and all(c["strides"].values()) and len(set(c["strides"].values())) == 6
                   for c in run if c["kernel"] == kernel)
    # every option of a call leaves its default in some case that runs
    for differs in (lambda c: c["bias"], lambda c: c["alpha"] != 1.0, lambda c: c["beta"] != 0.0, lambda c: c["relu"], lambda c: c["batch"] != 1,
                    lambda c: c["H"] != 1, lambda c: c["c_is_zero"], lambda c: c["colsum"], lambda c: c["m_dev"] is not None, lambda c: c["a_kpad"],
                    lambda c: c["a_rows"], *(lambda c, k=k: c["strides"][k] != 0 for k in ("sAb", "sAh", "sBb", "sBh", "sCb", "sCh"))):
        assert any(differs(c) for c in run)
    dma = [c for c in run if c["kernel"] == gc.DMA]
    for relu in (False, True):
        assert {c["f4"] for c in dma if c["relu"] == relu and c["bias"]} == {True, False}
    assert any(not c["f4"] and c["offC"] for c in dma) and any(not c["f4"] and c["ldc"] % 2 for c in dma) and any(not c["f4"] and c["beta"] == 1.0 for c in dma)
    # the sizes the issue lists, on the kernels that can take them
    sizes = [c for c in run if c["group"] == "sizes"]
    for kernel, Ms, Ns, Ks in ((gc.SMALL, {1, 47, 48, 50, 64, 65, 132}, {1, 47, 48, 49, 50, 51, 64, 68, 130}, {1, 4, 15, 16, 17, 20, 36, 172}),
                               (gc.BIG, {48, 50, 64, 65, 132}, {48, 49, 50, 51, 64, 68, 130}, {1, 4, 15, 16, 17, 20, 36, 172}),
                               (gc.DMA, {48, 50, 64, 65, 132}, {48, 49, 50, 51, 64, 68, 130}, {4, 16, 20, 36, 172})):
        mine = [c for c in sizes if c["kernel"] == kernel]
        assert ({c["M"] for c in mine}, {c["N"] for c in mine}, {c["K"] for c in mine}) == (Ms, Ns, Ks), kernel
    assert {c["N"] for c in sizes if c["kernel"] == gc.DMA and c["tB"]} >= {49, 50, 51}             # 1-, 2-, 3-column tail of the float4 epilogue
    assert all(c["M"] <= 200 and c["N"] <= 200 and c["K"] <= 2304 for c in gc.MM_CASES)
    assert {c["K"] for c in run if c["ksplit"] > 1} == {2048, 2050, 2052, 2304}
    rows = [c for c in run if c["a_rows"]]
    assert {(c["tB"], c["M"], c["m_dev"]) for c in rows if c["ksplit"] == 1} == {(tB, M, md) for tB in (True, False) for M in (48, 100)
                                                                                 for md in (None, 1, 64, 65, M) if md is None or md <= M}
    assert all(c["kernel"] == gc.DMA for c in rows)
    kp = [c for c in run if c["group"] == "kpad"]
    assert {(c["K"], c["a_kpad"], c["kernel"]) for c in kp} == {(K, f, k) for K in (18, 171) for f, k in ((True, gc.DMA), (False, gc.BIG))}
    assert all(by["data"] in {c["name"] for c in kp if c["a_kpad"]} for by in kp if not by["a_kpad"])
    for c in gc.MM_CASES:
        assert c["alpha"] in gc.ALPHAS and c["beta"] in gc.BETAS


def test_buffers_hold_nan_and_sentinels_outside_the_logical_elements():
    for c in gc.MM_CASES:
        a = gc.build(c, "exact")
        for X in "AB":
            inside = np.zeros(a[X].size, dtype=bool)
            inside[a["idx"][X].ravel()] = True
            assert np.isfinite(a[X][inside]).all() and inside.sum() > 0, (c["name"], X)
            outside = a[X][~inside]
            if X == "A" and c["zero_pad"]:
                assert (np.isnan(outside) | (outside == 0)).all() and (outside == 0).sum() == (gc.r4(c["K"]) - c["K"]) * c["M"], c["name"]
            else:
                assert np.isnan(outside).all(), (c["name"], X)
        inside = np.zeros(a["C"].size, dtype=bool)
        inside[a["idx"]["C"].ravel()] = True
        assert (a["C"].view(np.uint32)[~inside] == gc.SENTINEL_BITS).all() and (~inside).sum() >= 2 * 4 * c["ldc"], c["name"]
        if c["beta"] == 0.0 and not c["c_is_zero"]:
            assert (a["C"].view(np.uint32) == gc.SENTINEL_BITS).all(), c["name"]
        if c["a_rows"]:
            t = a["a_rows"]
            assert t.min() >= 0 and t.max() < c["M"] + 37 and len(set(t[:c["M"]].tolist())) < c["M"], c["name"]
        assert (a["base"]["A"] % 4, a["base"]["B"] % 4, a["base"]["C"] % 4) == (c["offA"], c["offB"], c["offC"])


@pytest.mark.parametrize("c", gc.MM_RUN, ids=gc.case_id)
def test_references_are_exact_in_float32_and_the_rounded_bound_binds(c):
    """Exact regime: the float64 reference of every case (and every column sum) is representable in float32 and below 2^24 -- asserted, as
    is the stronger fact that sum_k |alpha a b| + |bias| + |beta C0|, which bounds every partial sum in any order, stays below 2^24 with all
    terms multiples of 1/2.  Rounded regime: the bound is at most 1e-3 of max |ref| while K < 2048.  For standard normal operands the ratio
    is about 2 (K + 4) u * 0.64 K / (z sqrt(K)) = 7.6e-8 K^1.5 / z, z the largest of M N normal draws in units of sigma (3 .. 4.3 for the
    1040 .. 40000 outputs here, never below 2.5): it passes 1e-3 near K = 1000 whatever the seed and is 8.4e-3 / z at K = 2304, so the
    K >= 2048 cases are held to 4e-3 (the estimate at z = 2.5, with 5 % for the spread of the bound over the elements): an error of a
    single a b term, of order 1, is still twice the bound there, and the exact regime holds the same cases bit for bit.  The column sums of those cases
    (no cancellation help from B: |a| sums to 0.8 K, z ~ 2.5 over M <= 100 draws, ratio 4e-8 K^1.5 = 4.2e-3 at K = 2304) are held to 1e-2."""
    a = gc.build(c, "exact")
    r = gc.reference(c, a)
    ref = r["C"]
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref) and np.abs(ref).max() < 2 ** 24
    mag = r["C_bound"] / (2.0 * (c["K"] + 4) * gc.U)
    assert mag.max() < 2 ** 24 and np.array_equal(np.round(2 * ref), 2 * ref)
    if c["colsum"]:
        assert np.array_equal(r["colsum"].astype(np.float32).astype(np.float64), r["colsum"]) and np.abs(r["colsum"]).max() < 2 ** 24
    if c["relu"]:
        assert (ref == 0).any() and (ref > 0).any()                       # both sides of the kink are exercised
    r = gc.reference(c, gc.build(c, "rounded"))
    limit = 1e-3 if c["K"] < gc.SPLIT_K else 4e-3
    assert r["C_bound"].max() <= limit * np.abs(r["C"]).max(), (r["C_bound"].max(), np.abs(r["C"]).max())
    if c["colsum"]:
        limit = 1e-3 if c["K"] < gc.SPLIT_K else 1e-2
        assert r["colsum_bound"].max() <= limit * np.abs(r["colsum"]).max(), (r["colsum_bound"].max(), np.abs(r["colsum"]).max())


@pytest.mark.parametrize("case", gc.DW_CASES, ids=gc.case_id)
def test_dw_references_are_exact_or_bound(case):
    arrays = gc.dw_build(case)
    for r in gc.dw_reference(case, arrays):
        for key in ("C", "colsum"):
            if r[key] is None:
                continue
            if case["regime"] == "exact":
                assert np.array_equal(r[key].astype(np.float32).astype(np.float64), r[key]) and np.abs(r[key]).max() < 2 ** 24
                assert (r[key + "_bound"] / (2.0 * (case["K"] + 4) * gc.U)).max() < 2 ** 24
            else:
                assert r[key + "_bound"].max() <= 1e-3 * np.abs(r[key]).max()


def test_dw_table_covers_the_cross_and_the_five_problem_launch():
    assert {(c["K"], c["problems"][0]["M"], c["problems"][0]["N"]) for c in gc.DW_SINGLE} == {
        (K, M, N) for K in (1, 15, 16, 31, 32, 33, 200, 700) for M, N in ((4, 4), (30, 100), (128, 208), (132, 212), (260, 420))}
    assert gc.DW_SHAPES[1]["lda"] == 32
    five = gc.DW_FIVE["problems"]
    assert len(five) == 5 and len({(p["M"], p["N"]) for p in five}) == 5 and sum(p["colsum"] for p in five) == 2
    assert all(p["ldc"] > p["N"] for c in gc.DW_CASES for p in c["problems"])
    assert len(gc.DW_ROUNDED) == 3


@pytest.mark.parametrize("name", gc.SPOT_CASES)
def test_reference_agrees_with_torch_matmul_in_float64(name):
    c = next(c for c in gc.MM_CASES if c["name"] == name)
    a = gc.build(c, "rounded")
    opA, opB, C0, bias, _ = gc.operands(c, a)
    want = c["alpha"] * torch.matmul(torch.from_numpy(opA), torch.from_numpy(opB)) + torch.from_numpy(bias) + c["beta"] * torch.from_numpy(C0)
    if c["relu"]:
        want = torch.relu(want)
    got = gc.reference(c, a)["C"]
    assert got.shape == (c["batch"], c["M"], c["N"])
    np.testing.assert_allclose(got, want.numpy(), rtol=0, atol=1e-12)
    # ... and the operands are what the call's own addressing rule reads from the flat buffers
    rs = np.random.RandomState(1)
    st, base = c["strides"], a["base"]
    for _ in range(50):
        z, m, n, k = rs.randint(c["batch"]), rs.randint(c["M"]), rs.randint(c["N"]), rs.randint(c["K"])
        zb, zh = divmod(z, c["H"])
        pa = base["A"] + zb * st["sAb"] + zh * st["sAh"] + (k * c["lda"] + m if c["tA"] else m * c["lda"] + k)
        pb = base["B"] + zb * st["sBb"] + zh * st["sBh"] + (n * c["ldb"] + k if c["tB"] else k * c["ldb"] + n)
        assert a["A"][pa] == opA[z, m, k] and a["B"][pb] == opB[z, k, n]


def test_refusals_return_their_codes_without_a_gpu(lib, monkeypatch):
    """Fake, never followed pointers: a refusal that launched anything, or zeroed C first, would fault or report a HIP error instead."""
    from dyglib_amd import _capi
    for c in gc.MM_REFUSED:
        case_plan(lib, c, monkeypatch)
        args = _capi.MmArgs(**gc.fake_fields(c))
        assert lib.dygnn_mm(C.byref(args), None) == gc.E_UNSUPPORTED, c["name"]
        assert lib.dygnn_last_error().startswith(b"mm: "), c["name"]
    monkeypatch.delenv("DYGNN_MM_DMA", raising=False)
    ok = gc.fake_fields(next(c for c in gc.MM_CASES if c["name"] == "route-NT-eligible"))
    for change in (dict(A=None), dict(B=None), dict(C=None), dict(M=-1), dict(N=-1), dict(K=-1), dict(batch=-1), dict(H=0), dict(lda=3), dict(ldc=3)):
        args = _capi.MmArgs(**{**ok, **change})
        assert lib.dygnn_mm(C.byref(args), None) == gc.E_INVALID and lib.dygnn_mm_path(C.byref(args)) == gc.E_INVALID, change
    assert lib.dygnn_mm(None, None) == gc.E_INVALID
    for empty in (dict(M=0), dict(N=0), dict(batch=0)):                      # nothing to do: no launch, no error
        args = _capi.MmArgs(**{**ok, **empty})
        assert lib.dygnn_mm(C.byref(args), None) == 0 and lib.dygnn_mm_path(C.byref(args)) == 0
    for case in gc.DW_REFUSED:
        pairs = (_capi.DwPair * len(case["problems"]))(*[
            _capi.DwPair(gc.FAKE_BASE + 4 * p["offA"], p["lda"], p["M"], 2 * gc.FAKE_BASE, p["ldb"], p["N"], 3 * gc.FAKE_BASE, p["ldc"], None)
            for p in case["problems"]])
        assert lib.dygnn_dw_grouped(case["K"], pairs, len(case["problems"]), None) == gc.E_UNSUPPORTED, case["name"]
        assert lib.dygnn_last_error().startswith(b"dw_grouped: "), case["name"]
    one = (_capi.DwPair * 1)(_capi.DwPair(gc.FAKE_BASE, 8, 8, 2 * gc.FAKE_BASE, 8, 8, None, 8, None))
    assert lib.dygnn_dw_grouped(16, one, 1, None) == gc.E_INVALID
    assert lib.dygnn_dw_grouped(0, None, 0, None) == 0


def test_128_column_tiles_were_unreachable(lib, monkeypatch):
    """The deleted branch took k_mm_big's 128-column tile when !(N <= 64 || w64 * 0.95 < w128) with wT = ceil(N / T) * T / N.  Over every N
    the general GEMM can see here that never held (ceil(N / 128) * 128 is a multiple of 64 that is >= N, hence >= ceil(N / 64) * 64), in the
    double arithmetic the dispatch used; and every such N on an unaligned operand takes k_mm_big."""
    monkeypatch.delenv("DYGNN_MM_DMA", raising=False)
    c = dict(next(c for c in gc.MM_CASES if c["name"] == "route-NT-A+1"))
    for N in range(48, 2049):
        w64, w128 = float(-(-N // 64) * 64) / N, float(-(-N // 128) * 128) / N
        assert N <= 64 or w64 * 0.95 < w128, N
        f = gc.fake_fields({**c, "N": N, "ldc": N})
        assert plan(lib, f) == (gc.BIG, 1, 0), N
