"""The time encoder's cosine forms (csrc/time_encoding.h) run one by one through dygnn_timeenc_probe over the vector of
tests/time_encoding_cases.py and compared with cos / sin of float64(x).

The bar is the header's own promise, 7.5e-7 absolute = 2 pi * 1e-7 (reduction error below 1e-7 turns up to 3e7 rad) + 6e-8 (polynomial)
+ 2^-24 (rounding the result), and the same bar beyond 3e7, where libm's cosf / sinf (a few ulp) sit well inside it.  The equalities the
header states (cos_fast2 = cos_fast per lane, cos_time = cos_time_select everywhere, cos_time = cos_fast up to 3e7, even symmetry,
cos(+-0) = 1) are asserted bit for bit.  The observed maxima go to the run's summary (tests/parity.py)."""
import numpy as np
import pytest
import torch

from dyglib_amd import _capi
from tests import parity
from tests import time_encoding_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.0


def probe(form, x, pad=64):
    """out[i] = form(x[i]) on the GPU; the `pad` floats behind out[n] must come back untouched"""
    lib = _capi.load()
    n = len(x)
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)
    out = torch.full((n + pad,), SENTINEL, dtype=torch.float32, device=DEV)
    _capi.check(lib.dygnn_timeenc_probe(form, _capi.ptr(xd), n, _capi.ptr(out), _capi.current_stream_ptr()))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[n:] == SENTINEL).all(), (form, n)
    return got[:n]


@pytest.fixture(scope="module")
def cases():
    return tc.build()


@pytest.fixture(scope="module")
def outputs(cases):
    """every form over its whole domain, once for the module"""
    return {form: probe(form, cases.inputs(form)) for form in tc.FORMS}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def max_err(form, x, got):
    """max |got - f(float64(x))| over the finite x, and where"""
    fin = np.isfinite(x)
    assert np.isfinite(got[fin]).all(), tc.FORMS[form]
    err = np.abs(got[fin].astype(np.float64) - tc.reference(form, x[fin]))
    i = int(err.argmax())
    return float(err[i]), float(x[fin][i])


@pytest.mark.parametrize("form", list(tc.FORMS))
def test_accuracy_against_float64(form, cases, outputs):
    x, got = cases.inputs(form), outputs[form]
    worst = {}
    for name, s in cases.classes.items():
        if s.stop <= len(x) and name != "nonfinite":
            worst[name] = max_err(form, x[s], got[s])
    fast = max(worst[n][0] for n in worst if cases.classes[n].stop <= cases.n_fast)
    parity._record(f"time encoder {tc.FORMS[form]} vs float64, |x| <= 3e7 (bar 7.5e-7)", fast, 1.0, tc.BAR)
    if form in tc.GUARDED:
        libm = max(worst[n][0] for n in worst if cases.classes[n].start >= cases.n_fast)
        parity._record(f"time encoder {tc.FORMS[form]} vs float64, libm range (bar 7.5e-7)", libm, 1.0, tc.BAR)
        assert np.isnan(got[cases.classes["nonfinite"]]).all()          # +-inf and NaN come back as NaN
    print(tc.FORMS[form], {n: f"{e:.3e} at {at!r}" for n, (e, at) in worst.items()})
    for name, (e, at) in worst.items():
        assert e <= tc.BAR, f"{tc.FORMS[form]}, class {name}: |err| {e:.3e} > {tc.BAR:.1e} at x = {at!r}"


def test_cos_fast2_is_cos_fast_on_each_lane(cases, outputs):
    assert np.array_equal(bits(outputs[1]), bits(outputs[0]))
    # the same elements in the other lane, and paired with their other neighbour
    x = cases.inputs(1)
    order = np.arange(len(x)).reshape(-1, 2)[:, ::-1].reshape(-1)          # lanes swapped
    assert np.array_equal(bits(probe(1, x[order])), bits(outputs[0][order]))
    shifted = np.roll(x, 1)                                                # every element with its other neighbour
    assert np.array_equal(bits(probe(1, shifted)), bits(np.roll(outputs[0], 1)))


def test_cos_time_is_cos_time_select_everywhere(cases, outputs):
    fin = np.isfinite(cases.x)
    assert np.array_equal(bits(outputs[2][fin]), bits(outputs[3][fin]))          # the libm range included
    assert np.isnan(outputs[2][~fin]).all() and np.isnan(outputs[3][~fin]).all()


def test_guarded_forms_are_the_fast_forms_up_to_the_guard(cases, outputs):
    n = cases.n_fast
    assert np.array_equal(bits(outputs[2][:n]), bits(outputs[0]))
    assert np.array_equal(bits(outputs[3][:n]), bits(outputs[0]))
    assert np.array_equal(bits(outputs[5][:n]), bits(outputs[4]))


def test_cosine_is_even_and_one_at_zero(cases, outputs):
    x = cases.inputs(0)
    assert np.array_equal(bits(probe(0, -x)), bits(outputs[0]))
    assert np.array_equal(bits(probe(2, -cases.x[np.isfinite(cases.x)])), bits(outputs[2][np.isfinite(cases.x)]))
    zeros = np.array([0.0, -0.0], dtype=np.float32)
    for form in (0, 1, 2, 3):
        assert np.array_equal(bits(probe(form, zeros)), bits(np.ones(2, dtype=np.float32))), tc.FORMS[form]


def test_no_jump_where_the_two_paths_meet(cases, outputs):
    """3e7 (the fast path's last argument) and its upper neighbour (libm's first) are both within the bar of float64, in all guarded forms;
    cos and sin change by up to 2 between them (one ulp is 2 rad there), so the bar is on each value, not on their difference"""
    lo, hi = cases.classes["boundary_fast"], cases.classes["boundary_libm"]
    for form in tc.GUARDED:
        for s in (lo, hi):
            x, got = cases.x[s], outputs[form][s]
            err = np.abs(got.astype(np.float64) - tc.reference(form, x))
            assert (err <= tc.BAR).all(), (tc.FORMS[form], x[err.argmax()], err.max())
    edge = np.array([3e7, 30000002.0], dtype=np.float32)
    assert edge[1] == np.nextafter(edge[0], np.float32(np.inf))
    for form in tc.GUARDED:
        err = np.abs(probe(form, edge).astype(np.float64) - tc.reference(form, edge))
        parity._record(f"time encoder {tc.FORMS[form]} at 3e7 and its upper neighbour (bar 7.5e-7)", float(err.max()), 1.0, tc.BAR)
        assert (err <= tc.BAR).all(), (tc.FORMS[form], err)


@pytest.mark.parametrize("n", [1, 2, 63, 65, 257, 64 * 5 + 37])
def test_odd_sized_launches(n, cases, outputs):
    """n = 1, n below and above a wave and a block and no multiple of 64: the same bits as in the large launch, nothing written behind out[n]
    (probe() checks the pad); an odd n pairs cos_fast2's last element with 0"""
    at = cases.classes["sweep"].start + 1000
    for form in tc.FORMS:
        want = outputs[0 if form == 1 else form][at:at + n]
        assert np.array_equal(bits(probe(form, cases.x[at:at + n])), bits(want)), (tc.FORMS[form], n)


def test_empty_and_unknown_forms_launch_nothing():
    lib = _capi.load()
    assert lib.dygnn_timeenc_probe(0, None, 0, None, None) == 0               # empty: nothing launched
    assert lib.dygnn_timeenc_probe(6, None, 0, None, None) == -1 and lib.dygnn_timeenc_probe(-1, None, 0, None, None) == -1
