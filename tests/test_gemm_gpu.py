"""The general GEMM (dygnn_mm: k_mm, k_mm_big, k_mm_dma behind train::mm) and the grouped weight-gradient product (dygnn_dw_grouped) against
the float64 references of tests/gemm_cases.py, case by case: every kernel and orientation, both epilogues of k_mm_dma, split-K, the column
sums, the device-side row count, the row table, the a_kpad exemption and batched strides, at the sizes where each has a tail.

Each case runs in two value regimes (gemm_cases.py): "exact", where the bar is bitwise equality with the reference, and "rounded", where it
is the derived forward bound; the largest observed err / bound per kernel goes to the end-of-run table (tests.parity).  Operands are
surrounded by NaN and results by a sentinel bit pattern that must come back untouched; next to every launch the test asserts that
dygnn_mm_plan reports the kernel, the split and the epilogue the table intends."""
import ctypes as C

import numpy as np
import pytest
import torch

from dyglib_amd import _capi
from tests import gemm_cases as gc
from tests.parity import _record

pytestmark = pytest.mark.gpu


def _upload(arrays):
    dev = {k: torch.from_numpy(v).cuda() for k, v in arrays.items() if isinstance(v, np.ndarray)}
    assert all(t.data_ptr() % 16 == 0 for t in dev.values())
    return dev


def _set_env(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("DYGNN_MM_DMA", raising=False)
    else:
        monkeypatch.setenv("DYGNN_MM_DMA", value)


def run_mm(c, regime, monkeypatch, dma_env="case"):
    """One dygnn_mm call on a case's buffers.  Returns rc, the host arrays as built, the allocations as they came back, and the plan."""
    lib = _capi.load()
    _set_env(monkeypatch, c["dma_env"] if dma_env == "case" else dma_env)
    arrays = gc.build(c, regime)
    dev = _upload(arrays)
    args = _capi.MmArgs(**gc.mm_fields(c, {k: t.data_ptr() for k, t in dev.items()}, arrays))
    ks, f4 = C.c_int32(-7), C.c_int32(-7)
    kernel = lib.dygnn_mm_plan(C.byref(args), C.byref(ks), C.byref(f4))
    assert lib.dygnn_mm_path(C.byref(args)) == kernel
    rc = lib.dygnn_mm(C.byref(args), _capi.current_stream_ptr())
    torch.cuda.synchronize()
    return rc, arrays, {k: t.cpu().numpy() for k, t in dev.items()}, (kernel, ks.value, f4.value)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _compare(got, ref, bound, regime, what, label):
    if got.size == 0:
        return
    assert np.isfinite(got).all(), f"{what}: non-finite result"
    if regime == "exact":
        want = ref.astype(np.float32)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{what}: {len(bad)} elements differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"
        return
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"{what}: max err / bound = {ratio:.3g}")
    _record(label, ratio, float(np.abs(ref).max()), 1.0)
    assert (err <= bound).all(), f"{what}: err / bound up to {ratio:.3g} (max err {err.max():.3e})"


def check_mm(c, regime, arrays, got, kernel):
    """Results against the reference; everything the call may not write against what it held before the call."""
    r = gc.reference(c, arrays)
    M, live = c["M"], gc.live_rows(c)
    tile_end = min(M, -(-live // 64) * 64)                    # rows [live, tile_end) share a 64-row tile with live rows: not compared
    idx = arrays["idx"]["C"]
    name = gc.KERNEL_NAMES[kernel]
    _compare(got["C"][idx][:, :live], r["C"][:, :live], r["C_bound"][:, :live], regime, f"{c['name']} [{regime}] C", f"gemm {name}: err / bound")
    keep = np.ones(got["C"].size, dtype=bool)
    keep[idx[:, :tile_end].ravel()] = False
    assert np.array_equal(_bits(got["C"])[keep], _bits(arrays["C"])[keep]), f"{c['name']} [{regime}]: wrote outside its rows and columns of C"
    for X in ("A", "B", "bias", "a_rows", "m_dev"):
        if X in arrays:
            assert np.array_equal(_bits(got[X]), _bits(arrays[X])), (c["name"], X)
    if c["colsum"]:
        _compare(got["colsum"][16:16 + M], r["colsum"], r["colsum_bound"], regime, f"{c['name']} [{regime}] colsum", f"gemm {name}: colsum err / bound")
        keep = np.ones(got["colsum"].size, dtype=bool)
        keep[16:16 + M] = False
        assert np.array_equal(_bits(got["colsum"])[keep], _bits(arrays["colsum"])[keep]), f"{c['name']}: wrote outside colsum_out[0, M)"


@pytest.mark.parametrize("c", gc.MM_RUN, ids=gc.case_id)
def test_mm_matches_the_float64_reference(c, monkeypatch):
    for regime in ("exact", "rounded"):
        rc, arrays, got, (kernel, ks, f4) = run_mm(c, regime, monkeypatch)
        assert (kernel, ks, bool(f4)) == (c["kernel"], c["ksplit"], c["f4"]), (c["name"], kernel, ks, f4)
        _capi.check(rc)
        check_mm(c, regime, arrays, got, kernel)
    if not c["tA"] and c["tB"] and c["batch"] == 1:
        lib, f = _capi.load(), gc.fake_fields(c)
        assert lib.dygnn_mm_gathers_rows(f["A"], c["lda"], f["B"], c["ldb"], c["M"], c["N"], c["K"]) == int(kernel == gc.DMA)


@pytest.mark.parametrize("c", gc.MM_REFUSED, ids=gc.case_id)
def test_mm_refuses_before_it_launches_or_zeroes_anything(c, monkeypatch):
    rc, arrays, got, (kernel, _, _) = run_mm(c, "exact", monkeypatch)
    assert rc == kernel == gc.E_UNSUPPORTED
    with pytest.raises(NotImplementedError, match="mm: "):
        _capi.check(rc)
    for X, before in arrays.items():
        if isinstance(before, np.ndarray):
            assert np.array_equal(_bits(got[X]), _bits(before)), (c["name"], X)


def _live(c, arrays, got):
    out = [got["C"][arrays["idx"]["C"]][:, :gc.live_rows(c)]]
    if c["colsum"]:
        out.append(got["colsum"])
    return out


DMA_ELIGIBLE = [c for c in gc.MM_RUN if c["kernel"] == gc.DMA and not c["a_rows"]]


@pytest.mark.parametrize("group", sorted({c["group"] for c in DMA_ELIGIBLE}))
def test_the_dma_switch_changes_the_kernel_and_not_a_bit(group, monkeypatch):
    """DYGNN_MM_DMA=0 (read per call) sends every DMA-eligible case to k_mm_big; in the exact regime the results agree bit for bit."""
    for c in (c for c in DMA_ELIGIBLE if c["group"] == group):
        rc1, arrays, on, (k1, ks1, _) = run_mm(c, "exact", monkeypatch, dma_env=None)
        rc0, _, off, (k0, ks0, f40) = run_mm(c, "exact", monkeypatch, dma_env="0")
        assert (rc1, rc0, k1, k0, f40) == (0, 0, gc.DMA, gc.BIG, 0) and ks1 == ks0 == c["ksplit"], c["name"]
        for a, b in zip(_live(c, arrays, on), _live(c, arrays, off)):
            assert np.array_equal(_bits(a), _bits(b)), c["name"]
        check_mm(c, "exact", arrays, off, k0)


@pytest.mark.parametrize("kernel", [gc.SMALL, gc.BIG, gc.DMA], ids=lambda k: gc.KERNEL_NAMES[k])
def test_a_split_product_run_twice_gives_the_same_bits(kernel, monkeypatch):
    for c in (c for c in gc.MM_RUN if c["kernel"] == kernel and c["ksplit"] > 1 and c["group"] in ("splitk", "colsum")):
        _, arrays, first, _ = run_mm(c, "exact", monkeypatch)
        _, _, second, plan = run_mm(c, "exact", monkeypatch)
        assert plan[1] == c["ksplit"] > 1
        for X in first:
            assert np.array_equal(_bits(first[X]), _bits(second[X])), (c["name"], X)


def test_a_kpad_only_picks_the_kernel(monkeypatch):
    """The same buffers with and without the flag: k_mm_dma and k_mm_big, the same bits (exact regime)."""
    by_name = {c["name"]: c for c in gc.MM_RUN}
    pairs = [(by_name[c["data"]], c) for c in gc.MM_RUN if c["group"] == "kpad" and not c["a_kpad"]]
    assert len(pairs) == 4
    for flag, noflag in pairs:
        _, a1, g1, p1 = run_mm(flag, "exact", monkeypatch)
        _, a0, g0, p0 = run_mm(noflag, "exact", monkeypatch)
        assert (p1[0], p0[0]) == (gc.DMA, gc.BIG) and np.array_equal(_bits(a1["A"]), _bits(a0["A"])) and np.array_equal(_bits(a1["B"]), _bits(a0["B"]))
        assert np.array_equal(_bits(g1["C"]), _bits(g0["C"])), flag["name"]


# ---- dw_grouped ---------------------------------------------------------------------------------------------------------------------------------
def run_dw(case):
    lib = _capi.load()
    arrays = gc.dw_build(case)
    devs = [_upload(a) for a in arrays]
    pairs = (_capi.DwPair * len(arrays))(*[
        _capi.DwPair(d["A"].data_ptr() + 4 * a["base"]["A"], p["lda"], p["M"], d["B"].data_ptr() + 4 * a["base"]["B"], p["ldb"], p["N"],
                     d["C"].data_ptr() + 4 * a["base"]["C"], p["ldc"], d["colsum"].data_ptr() + 4 * a["base"]["colsum"] if p["colsum"] else None)
        for p, a, d in zip(case["problems"], arrays, devs)])
    rc = lib.dygnn_dw_grouped(case["K"], pairs, len(arrays), _capi.current_stream_ptr())
    torch.cuda.synchronize()
    return rc, arrays, [{k: t.cpu().numpy() for k, t in d.items()} for d in devs]


@pytest.mark.parametrize("case", gc.DW_CASES, ids=gc.case_id)
def test_dw_grouped_accumulates_the_float64_reference(case):
    rc, arrays, got = run_dw(case)
    _capi.check(rc)
    for i, (p, a, g, r) in enumerate(zip(case["problems"], arrays, got, gc.dw_reference(case, arrays))):
        what = f"{case['name']} problem {i}"
        _compare(g["C"][a["idx"]["C"]], r["C"], r["C_bound"], case["regime"], what + " C", "gemm k_dw_grouped: err / bound")
        keep = np.ones(g["C"].size, dtype=bool)
        keep[a["idx"]["C"].ravel()] = False
        assert np.array_equal(_bits(g["C"])[keep], _bits(a["C"])[keep]), what + ": wrote outside C[M][N]"
        assert np.array_equal(_bits(g["A"]), _bits(a["A"])) and np.array_equal(_bits(g["B"]), _bits(a["B"]))
        if p["colsum"]:
            M = p["M"]
            _compare(g["colsum"][16:16 + M], r["colsum"], r["colsum_bound"], case["regime"], what + " colsum", "gemm k_dw_grouped: colsum err / bound")
            keep = np.ones(g["colsum"].size, dtype=bool)
            keep[16:16 + M] = False
            assert np.array_equal(_bits(g["colsum"])[keep], _bits(a["colsum"])[keep]), what + ": wrote outside colsum[0, M)"


@pytest.mark.parametrize("case", gc.DW_REFUSED, ids=gc.case_id)
def test_dw_grouped_refuses_before_it_launches(case):
    rc, arrays, got = run_dw(case)
    assert rc == gc.E_UNSUPPORTED
    with pytest.raises(NotImplementedError, match="dw_grouped: "):
        _capi.check(rc)
    for a, g in zip(arrays, got):
        for X in ("A", "B", "C", "colsum"):
            assert np.array_equal(_bits(g[X]), _bits(a[X])), (case["name"], X)
