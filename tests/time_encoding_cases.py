"""The input vector of the time-encoder cosine probe (dygnn_timeenc_probe, csrc/time_encoding_probe.hip): one seeded float32 vector of about
2^20 elements, built class by class.  numpy only: tests/test_time_encoding_cases_cpu.py checks the vector without a GPU,
tests/test_time_encoding_gpu.py runs every form of csrc/time_encoding.h over it and compares with float64.

The first `n_fast` elements are the domain of the unguarded forms (cos_fast, cos_fast2, sin_fast): nothing beyond kFastMax = 3e7, nothing that
is not finite.  The guarded forms (cos_time, cos_time_select, sin_time) take the whole vector."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict

import numpy as np

FAST_MAX = np.float32(3.0e7)           # time_encoding.h: kFastMax
# the header's own promise: 2 pi * 1e-7 (reduction, in turns) + 6e-8 (polynomial) + 2^-24 (rounding the result) = 7.48e-7
BAR = 7.5e-7

FORMS = {0: "cos_fast", 1: "cos_fast2", 2: "cos_time", 3: "cos_time_select", 4: "sin_fast", 5: "sin_time"}
GUARDED = (2, 3, 5)
SINES = (4, 5)

SEED = 20261
SWEEP_PER_SIGN = 1 << 17               # log-uniform magnitudes in [1e-8, 3e7]
PI_DENSE = 4096                        # every k below this
PI_SEEDED = 200_000                    # seeded k in [PI_DENSE, PI_MAX_K]
PI_MAX_K = 19_000_000                  # 1.9e7 * pi / 2 = 2.98e7 < 3e7
BEYOND_SWEEP = 2048                    # log-uniform magnitudes in (3e7, 3e9]: where UNIX-epoch timestamps put the highest frequencies
BEYOND_NAMED = (3.1e7, 1e9, 2.7e9, 1e30, float(np.finfo(np.float32).max))


@dataclass(frozen=True)
class Cases:
    x: np.ndarray                      # float32 [n]
    classes: Dict[str, slice]          # class name -> its elements of x
    n_fast: int                        # x[:n_fast] is the domain of forms 0, 1 and 4

    def inputs(self, form: int) -> np.ndarray:
        return self.x if form in GUARDED else self.x[:self.n_fast]


def _ulp_neighbours(v: np.ndarray) -> np.ndarray:
    """[n] float32 -> [n, 5]: v - 2 ulp, v - 1 ulp, v, v + 1 ulp, v + 2 ulp"""
    lo1 = np.nextafter(v, np.float32(-np.inf))
    hi1 = np.nextafter(v, np.float32(np.inf))
    return np.stack([np.nextafter(lo1, np.float32(-np.inf)), lo1, v, hi1, np.nextafter(hi1, np.float32(np.inf))], axis=1)


def _log_uniform(rs, lo, hi, n):
    return np.exp(rs.uniform(np.log(lo), np.log(hi), size=n))


def build(seed: int = SEED) -> Cases:
    rs = np.random.RandomState(seed)
    parts, classes, at = [], {}, 0

    def add(name, v):
        nonlocal at
        v = np.ascontiguousarray(v, dtype=np.float32).reshape(-1)
        parts.append(v)
        classes[name] = slice(at, at + len(v))
        at += len(v)

    # log-uniform sweeps, both signs, independent draws: consecutive elements (the pairs of cos_fast2) land in unrelated branches
    mag = np.minimum(_log_uniform(rs, 1e-8, 3e7, 2 * SWEEP_PER_SIGN).astype(np.float32), FAST_MAX)
    sign = np.where(np.arange(2 * SWEEP_PER_SIGN) % 4 < 2, 1.0, -1.0).astype(np.float32)      # as many of each sign, shuffled: pairs of equal
    add("sweep", mag * sign[rs.permutation(2 * SWEEP_PER_SIGN)])                                # and of opposite sign
    # multiples of pi / 2 and their neighbours: fold edges (u = 0.25, 0.5), zero crossings, extrema
    k = np.arange(PI_DENSE, dtype=np.float64)
    dense = _ulp_neighbours((k * (np.pi / 2)).astype(np.float32))
    add("pi_dense", np.concatenate([dense, -dense]))
    k = rs.randint(PI_DENSE, PI_MAX_K + 1, size=PI_SEEDED).astype(np.float64)
    seeded = _ulp_neighbours((k * (np.pi / 2)).astype(np.float32))
    add("pi_seeded", seeded * np.where(rs.randint(0, 2, size=(PI_SEEDED, 1)) == 1, np.float32(1), np.float32(-1)))
    # the guard boundary, the side the fast path takes: 3e7 and its two lower neighbours
    edge = _ulp_neighbours(np.array([FAST_MAX], dtype=np.float32))[0]
    add("boundary_fast", np.concatenate([edge[:3], -edge[:3]]))
    tiny = np.float32(np.finfo(np.float32).tiny)
    denormals = np.array([1e-45, 1e-40, 5.9e-39], dtype=np.float32)
    add("specials", np.concatenate([[np.float32(0.0), np.float32(-0.0), tiny, -tiny], denormals, -denormals]))
    n_fast = at
    # ---- guarded forms only
    add("boundary_libm", np.concatenate([edge[3:], -edge[3:]]))
    named = np.array(BEYOND_NAMED, dtype=np.float32)
    add("beyond_named", np.concatenate([named, -named]))
    far = np.maximum(_log_uniform(rs, 3e7, 3e9, BEYOND_SWEEP).astype(np.float32), edge[3])
    add("beyond_sweep", far * np.where(rs.randint(0, 2, size=BEYOND_SWEEP) == 1, np.float32(1), np.float32(-1)))
    add("nonfinite", np.array([np.inf, -np.inf, np.nan], dtype=np.float32))
    return Cases(x=np.concatenate(parts), classes=classes, n_fast=n_fast)


def reference(form: int, x: np.ndarray) -> np.ndarray:
    """cos (or sin) of float64(x): the bar's other side"""
    with np.errstate(invalid="ignore"):
        return (np.sin if form in SINES else np.cos)(x.astype(np.float64))


def turns_fraction64(x: np.ndarray) -> np.ndarray:
    """x / (2 pi) minus the nearest integer, in float64 (good to ~1e-9 turns at 3e7 rad): which branches an argument takes"""
    t = x.astype(np.float64) / (2 * np.pi)
    return t - np.rint(t)
