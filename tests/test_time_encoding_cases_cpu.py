"""Conditions on the input vector of tests/time_encoding_cases.py (no GPU): it is deterministic, every class the probe test relies on is
present in a stated number, and the unguarded forms' part holds nothing beyond kFastMax."""
import re
import os

import numpy as np

from tests import time_encoding_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = tc.build()
X64 = C.x.astype(np.float64)


def _cls(name):
    return C.x[C.classes[name]]


def test_the_builder_is_deterministic_and_the_classes_tile_the_vector():
    again = tc.build()
    assert C.x.dtype == np.float32 and C.x.ndim == 1
    assert np.array_equal(C.x.view(np.uint32), again.x.view(np.uint32)) and again.classes == C.classes and again.n_fast == C.n_fast
    assert not np.array_equal(tc.build(tc.SEED + 1).x.view(np.uint32), C.x.view(np.uint32))
    at = 0
    for s in C.classes.values():          # consecutive, nothing unnamed
        assert s.start == at and s.stop > s.start
        at = s.stop
    assert at == len(C.x)
    assert 0.9 * 2 ** 20 <= len(C.x) <= 1.5 * 2 ** 20
    assert C.classes["specials"].stop == C.n_fast == C.classes["boundary_libm"].start
    assert C.n_fast % 2 == 0               # cos_fast2's pairs are whole


def test_the_constants_are_the_headers():
    header = open(os.path.join(ROOT, "dyglib_amd", "csrc", "time_encoding.h")).read()
    assert np.float32(float(re.search(r"kFastMax = ([0-9.e+]+)f", header).group(1))) == tc.FAST_MAX
    assert abs(tc.BAR - (2 * np.pi * 1e-7 + 6e-8 + 2.0 ** -24)) < 3e-9


def test_the_unguarded_part_stays_inside_the_fast_range():
    fast = C.x[:C.n_fast]
    assert np.isfinite(fast).all() and np.abs(fast).max() == tc.FAST_MAX
    for form in tc.FORMS:
        assert len(C.inputs(form)) == (len(C.x) if form in tc.GUARDED else C.n_fast)
    rest = C.x[C.n_fast:]
    assert (~np.isfinite(rest) | (np.abs(rest) > tc.FAST_MAX)).all()          # and the rest is all beyond it: only the guard keeps it from cos_fast


def test_log_uniform_sweeps():
    s = _cls("sweep")
    assert len(s) == 2 * tc.SWEEP_PER_SIGN >= 1 << 18
    assert (s > 0).sum() == (s < 0).sum() == tc.SWEEP_PER_SIGN
    a = np.abs(s)
    assert a.min() >= np.float32(1e-8) and a.max() <= tc.FAST_MAX
    counts, _ = np.histogram(np.log10(a), bins=np.arange(-8.0, 9.0))          # decades from 1e-8, the last one cut at 3e7
    assert counts.sum() == len(s) and (counts[:-1] >= 14_000).all() and counts[-1] >= 6_000, counts
    assert ((a > 2.7e6) & (a <= 3e7)).sum() >= 15_000                          # the decade no fixture graph reaches


def test_multiples_of_half_pi_with_their_neighbours():
    half_pi = np.pi / 2
    for name, n_k, signs in (("pi_dense", tc.PI_DENSE, 2), ("pi_seeded", tc.PI_SEEDED, 1)):
        v = _cls(name).reshape(signs * n_k, 5)
        mid = v[:, 2].astype(np.float64)
        k = np.rint(np.abs(mid) / half_pi)
        assert (np.abs(mid).astype(np.float32) == (k * half_pi).astype(np.float32)).all(), name          # the centre IS float32(k pi / 2)
        a = np.abs(v)                                                                                      # a negated row keeps its order in magnitude
        nz = k > 0
        assert (np.diff(a[nz], axis=1) > 0).all(), name
        for j in range(4):                                                                                 # consecutive floats: 1 ulp apart
            assert (np.nextafter(a[nz, j], np.float32(np.inf)) == a[nz, j + 1]).all(), (name, j)
    dense = _cls("pi_dense").reshape(2, tc.PI_DENSE, 5)
    assert np.array_equal(np.rint(dense[0, :, 2].astype(np.float64) / half_pi), np.arange(tc.PI_DENSE))      # every k < 4096 ...
    assert np.array_equal(dense[1], -dense[0])                                                               # ... with both signs
    seeded = _cls("pi_seeded").reshape(tc.PI_SEEDED, 5)
    k = np.rint(np.abs(seeded[:, 2].astype(np.float64)) / half_pi).astype(np.int64)
    assert tc.PI_SEEDED >= 200_000 and k.min() >= tc.PI_DENSE and 1.85e7 < k.max() <= 1.9e7 and len(np.unique(k)) > 0.98 * tc.PI_SEEDED
    for r in range(4):                                                                                       # zero crossings and both extrema
        assert (k % 4 == r).sum() >= 45_000, r
    assert min((seeded[:, 2] > 0).sum(), (seeded[:, 2] < 0).sum()) >= 90_000
    assert np.abs(seeded).max() < tc.FAST_MAX
    # what the dense ones are for: arguments within an ulp or two of the fold edges u = 0.25 (odd k) and u = 0.5 (k = 2 mod 4).  (One float32
    # ulp is 7.8e-5 turns at k = 4095; the seeded k are rounded by up to a radian and land anywhere in the period.)
    u = np.abs(tc.turns_fraction64(dense[0]))
    assert (np.abs(u - 0.25) < 2.5e-4).sum() == 5 * tc.PI_DENSE // 2 and (np.abs(u - 0.5) < 2.5e-4).sum() == 5 * tc.PI_DENSE // 4


def test_guard_boundary_and_specials():
    lo, hi = _cls("boundary_fast"), _cls("boundary_libm")
    assert sorted(lo.tolist()) == [-3e7, -29999998.0, -29999996.0, 29999996.0, 29999998.0, 3e7]
    assert sorted(hi.tolist()) == [-30000004.0, -30000002.0, 30000002.0, 30000004.0]
    sp = _cls("specials")
    zeros = sp[sp == 0]
    assert len(zeros) == 2 and np.signbit(zeros).sum() == 1
    tiny = np.finfo(np.float32).tiny
    assert (np.abs(sp) == tiny).sum() == 2
    den = sp[(sp != 0) & (np.abs(sp) < tiny)]
    assert len(den) >= 6 and (den > 0).sum() == (den < 0).sum() and np.float32(1e-45) in den          # the smallest denormal among them


def test_the_guarded_forms_part():
    named = _cls("beyond_named")
    for v in tc.BEYOND_NAMED:
        assert (named == np.float32(v)).sum() == 1 and (named == -np.float32(v)).sum() == 1, v
    assert set(np.float32(v) for v in (3.1e7, 1e9, 2.7e9, 1e30, np.finfo(np.float32).max)) <= set(named.tolist())
    far = _cls("beyond_sweep")
    assert len(far) >= 2048 and np.abs(far).min() > tc.FAST_MAX and np.abs(far).max() <= np.float32(3e9)
    assert min((far > 0).sum(), (far < 0).sum()) >= 900
    nf = _cls("nonfinite")
    assert np.isposinf(nf).sum() == 1 and np.isneginf(nf).sum() == 1 and np.isnan(nf).sum() == 1
    assert np.isfinite(C.x).sum() == len(C.x) - 3


def test_pairs_of_cos_fast2_take_different_branches():
    """consecutive elements (x[2i], x[2i + 1]) whose two lanes differ in the sign of the turns fraction (the fabsf) and in the fold to
    [0, 0.25] (the flip and the final sign): margins of 1e-4 turns keep float64's view of the branch the kernel's"""
    fr = tc.turns_fraction64(C.x[:C.n_fast]).reshape(-1, 2)
    clear = (np.abs(np.abs(fr) - 0.25) > 1e-4).all(axis=1) & (np.abs(fr) > 1e-4).all(axis=1) & (np.abs(fr) < 0.5 - 1e-4).all(axis=1)
    flip = np.abs(fr) > 0.25
    neg = fr < 0
    assert (clear & (flip[:, 0] != flip[:, 1])).sum() >= 20_000
    assert (clear & (neg[:, 0] != neg[:, 1])).sum() >= 20_000
    assert (clear & (flip[:, 0] != flip[:, 1]) & (neg[:, 0] != neg[:, 1])).sum() >= 5_000
    assert (clear & (flip[:, 0] == flip[:, 1]) & (neg[:, 0] == neg[:, 1])).sum() >= 5_000


def test_the_reference_is_float64_of_the_float32_argument():
    x = np.array([1.0, 3e7, -2.7e9, 1e30], dtype=np.float32)
    assert np.array_equal(tc.reference(0, x), np.cos(x.astype(np.float64))) and np.array_equal(tc.reference(5, x), np.sin(x.astype(np.float64)))
    assert tc.reference(2, x).dtype == np.float64
    assert np.isnan(tc.reference(2, _cls("nonfinite"))).all()
