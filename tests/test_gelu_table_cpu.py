"""The GELU table of the fused DyGFormer inference kernels (csrc/gelu_table.h) on the host.

* The table as the packed buffer holds it (dygnn_gelu_table_host) against float64 math.erf: every knot is Phi(x_i) rounded once, cell 0
  starts at exactly 0 (Phi = 0 at and below -6), the last cell ends at exactly 1.0f, the knots never decrease, and a cell's base + step
  lies within one ulp of the next cell's base (it IS the next base: the step is the exact difference of the rounded knots).
* The table form in numpy fp32 — the device function's arithmetic, operation for operation — on 4 M arguments (uniform in [-8, 8] and
  N(0, 1.5)): its largest |gelu - exact| is the 4.82e-7 the table size was chosen by, to two digits.
* The host function alone in a stand-alone program (tools/gelu_table_check.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from dyglib_amd import _build, _capi

CELLS = 4096
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lib_table():
    out = np.full((CELLS + 1, 2), np.nan, dtype=np.float32)          # one guard row behind the table
    assert _capi.load().dygnn_gelu_table_host(out.ctypes.data) == 0
    assert np.isnan(out[CELLS]).all(), "gelu_table_host wrote past 4096 cells"
    assert np.isfinite(out[:CELLS]).all()
    return out[:CELLS, 0].copy(), out[:CELLS, 1].copy()


def phi64(x):
    return 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))


def test_null_pointer_is_an_error():
    assert _capi.load().dygnn_gelu_table_host(None) != 0


def test_probe_rejects_bad_arguments_before_it_launches():
    lib = _capi.load()
    assert lib.dygnn_gelu_probe(None, None, 0, 0, None) == 0                          # empty: nothing launched
    assert lib.dygnn_gelu_probe(None, None, 0, 2, None) == -1 and lib.dygnn_gelu_probe(None, None, 0, -1, None) == -1
    assert lib.dygnn_gelu_probe(None, None, 4, 0, None) == -1 and lib.dygnn_gelu_probe(None, None, -1, 0, None) == -1


def test_table_contents_against_float64_erf():
    base, step = lib_table()
    knots = np.array([phi64(-6.0 + 12.0 * i / CELLS) for i in range(CELLS + 1)])
    assert base[0] == 0.0 and not np.signbit(base[0])                                  # Phi(-6) = 9.9e-10 is forced to 0
    assert np.array_equal(base[1:], knots[1:CELLS].astype(np.float32))                 # rounded once
    top = np.float32(base[-1] + step[-1])
    assert top == np.float32(1.0) and np.float32(knots[CELLS]) == np.float32(1.0)      # exactly 1 at the top
    assert (step >= 0).all() and (np.diff(base) >= 0).all()                            # monotone
    # base[i] + step[i] (one fp32 addition, as the kernel's fma at fraction 1 would form it) within 1 ulp of base[i + 1]
    nxt = np.append(base[1:], np.float32(1.0))
    ends = (base + step).astype(np.float32)
    assert (np.abs(ends.astype(np.float64) - nxt.astype(np.float64)) <= np.spacing(nxt).astype(np.float64)).all()
    # and the step is the float64 difference of the knots to the two roundings of its ends (2 x 2^-25), cell 0 apart (its base is moved to 0)
    d64 = np.diff(knots)
    assert np.abs(step[1:].astype(np.float64) - d64[1:]).max() <= 2.0 ** -24
    assert abs(float(step[0]) - knots[1]) <= 2.0 ** -24


def gelu_table_numpy(v, base, step):
    """fused3_device.h: gelu_table, in fp32 operation for operation (an fma is the float64 product and sum rounded once: the product of two
    fp32 values is exact in float64)."""
    f32, f64 = np.float32, np.float64
    v = v.astype(f32)
    t = (v.astype(f64) * f64(f32(CELLS / 12.0)) + 2048.0).astype(f32)                  # fma(v, cells per unit, 2048)
    t = np.minimum(np.maximum(t, f32(0)), np.nextafter(f32(CELLS), f32(0)))            # v_med3 to [0, the largest float below 4096]
    i = t.astype(np.int32)                                                             # v_cvt_i32: truncation
    fr = (t - i.astype(f32)).astype(f32)                                               # v_fract (exact)
    phi = (fr.astype(f64) * step[i].astype(f64) + base[i].astype(f64)).astype(f32)     # fma(fraction, step, base)
    return (v * phi).astype(f32)


def test_table_form_in_numpy_reproduces_the_error_the_size_was_chosen_by():
    base, step = lib_table()
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.uniform(-8, 8, 2_000_000), rng.normal(0, 1.5, 2_000_000)]).astype(np.float32)
    v64 = torch.from_numpy(v.astype(np.float64))
    exact = (0.5 * v64 * (1.0 + torch.erf(v64 / math.sqrt(2.0)))).numpy()
    err = np.abs(gelu_table_numpy(v, base, step).astype(np.float64) - exact)
    k = int(err.argmax())
    print(f"table form, numpy fp32, 4 M arguments: max |gelu - exact| = {err.max():.3e} at v = {v[k]:.6f}")
    assert abs(err.max() - 4.82e-7) <= 0.05e-7, err.max()                              # 4.82e-7 to two digits


def test_stand_alone_host_program_under_asan_and_ubsan(tmp_path):
    # the clang++ that hipcc drives (ROCm's), else whatever host compiler there is: the program needs no HIP
    rocm_clang = os.path.join(os.path.dirname(os.path.realpath(_build._hipcc())), "..", "lib", "llvm", "bin", "clang++")
    cxx = next((c for c in (rocm_clang, shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "gelu_table_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", _build.CSRC, os.path.join(ROOT, "tools", "gelu_table_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 0 and "gelu_table_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
