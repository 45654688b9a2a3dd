"""Conditions on the inputs of tests/merge_layer_cases.py (not measurements of the library; no GPU): the bars of
tests/test_merge_layer_gpu.py only mean what they say while these hold."""
import numpy as np
import pytest
import torch

from dyglib_amd import MergeLayer
from tests import merge_layer_cases as mc


def test_case_table_has_every_width_and_row_count_it_promises():
    assert len(set(mc.FORWARD_CASES)) == len(mc.FORWARD_CASES) and len(set(mc.BACKWARD_CASES)) == len(mc.BACKWARD_CASES)
    by_width = {}
    for dim, hidden, n, path, kind in mc.FORWARD_CASES:
        by_width.setdefault((dim, hidden), {}).setdefault(path, set()).add(n)
    for w in mc.ROW_BLOCK_WIDTHS:
        assert w[0] % 4 == 0 and w[1] <= 256
        assert by_width[w] == {p: set(mc.N_OF_PATH[p]) for p in (mc.G, mc.R1, mc.R4)}, w
    for w in mc.MFMA_WIDTHS:
        assert w[0] % 4 == 0 and w[1] > 256
        assert by_width[w] == {mc.G: set(mc.N_OF_PATH[mc.G]) | {2047}, mc.M: set(mc.N_OF_PATH[mc.M])}, w
    assert by_width[(170, 172)] == {mc.G: {1, 63, 2100}}
    assert by_width[(516, 4)] == {mc.R1: {2047, 2048}} and by_width[(4100, 4)] == {mc.G: {63, 64}, mc.M: {2048}}
    assert {c[3] for c in mc.FORWARD_CASES} == {mc.G, mc.R1, mc.R4, mc.M}
    # ragged ends: 1 and 3 of 4 rows, 1 and 15 of 16 rows / of a wave, 3 of 4 live waves
    assert {n % 4 for n in mc.RAGGED_N[mc.R1]} == {1, 3} and {n % 16 for n in mc.RAGGED_N[mc.R4]} == {1, 15}
    assert {n % 16 for n in mc.RAGGED_N[mc.M]} >= {1, 15} and {(n + 15) // 16 % 4 for n in mc.RAGGED_N[mc.M]} >= {1, 3, 0}
    for path, ns in mc.RAGGED_N.items():
        assert set(ns) <= set(mc.N_OF_PATH[path])
    for dim, hidden, n, kind in mc.BACKWARD_CASES:
        assert dim % 4 == 0 and hidden % 4 == 0 and hidden <= 192
    assert {c[:2] for c in mc.BACKWARD_CASES} == set(mc.BACKWARD_WIDTHS) and {c[2] for c in mc.BACKWARD_CASES} == set(mc.BACKWARD_N)


def test_parameters_are_drawn_like_nn_linear():
    for dim, hidden in mc.ROW_BLOCK_WIDTHS + mc.MFMA_WIDTHS + mc.BACKWARD_WIDTHS:
        p = mc.params(dim, hidden)
        k1, k2 = 1 / np.sqrt(2 * dim), 1 / np.sqrt(hidden)
        assert p["fc1.weight"].shape == (hidden, 2 * dim) and p["fc1.bias"].shape == (hidden,)
        assert p["fc2.weight"].shape == (1, hidden) and p["fc2.bias"].shape == (1,)
        assert all(v.dtype == np.float32 for v in p.values())
        assert np.abs(p["fc1.weight"]).max() <= k1 and np.abs(p["fc1.bias"]).max() <= k1 and np.abs(p["fc2.weight"]).max() <= k2
        if hidden * dim >= 64:                                    # the draws fill their interval
            assert np.abs(p["fc1.weight"]).max() > 0.8 * k1


@pytest.mark.parametrize("case", [(12, 20, 33, "nn"), (172, 172, 17, "syn7")], ids=mc.case_id)
def test_reference_is_the_module_in_float64(case):
    """The numpy forward and the autograd expression of merge_layer_cases are MergeLayer (models/modules.py:57-68) evaluated in float64."""
    dim, hidden, n, kind = case
    a, b, g = mc.backward_inputs(*case)
    p = mc.params(dim, hidden, kind)
    m = MergeLayer(dim, dim, hidden, 1).double()
    m.load_state_dict({k: torch.from_numpy(np.array(v)).double() for k, v in p.items()})
    ta, tb = torch.from_numpy(np.array(a)).double().requires_grad_(True), torch.from_numpy(np.array(b)).double().requires_grad_(True)
    z = m(ta, tb)
    (z[:, 0] * torch.from_numpy(np.array(g)).double()).sum().backward()
    ref = mc.backward_reference(*case)
    zf, pf = mc.reference_forward(a, b, p)
    np.testing.assert_allclose(zf, z.detach().numpy()[:, 0], rtol=0, atol=1e-13)
    np.testing.assert_allclose(pf, torch.sigmoid(z).detach().numpy()[:, 0], rtol=0, atol=1e-13)
    np.testing.assert_allclose(ref["z"], zf, rtol=0, atol=1e-13)
    np.testing.assert_allclose(ref["a"], ta.grad.numpy(), rtol=0, atol=1e-13)
    np.testing.assert_allclose(ref["b"], tb.grad.numpy(), rtol=0, atol=1e-13)
    for k, q in (("w1", m.fc1.weight), ("b1", m.fc1.bias), ("w2", m.fc2.weight), ("b2", m.fc2.bias)):
        np.testing.assert_allclose(ref[k], q.grad.numpy(), rtol=0, atol=1e-12)


@pytest.mark.parametrize("case", mc.BACKWARD_CASES, ids=mc.case_id)
def test_backward_pre_activations_keep_their_distance_from_the_relu_kink(case):
    """A float32 pre-activation within rounding of 0 may take the other side of the ReLU than the float64 reference: a gradient then differs by a
    whole g * w2 term with no error in the kernel.  The seeds are chosen so that no pre-activation is that close."""
    dim, hidden, n, kind = case
    a, b, _ = mc.backward_inputs(*case)
    pre = mc.reference_pre(a, b, mc.params(dim, hidden, kind))
    assert pre.shape == (n, hidden)
    assert np.abs(pre).min() >= mc.PRE_MARGIN, np.abs(pre).min()


@pytest.mark.parametrize("case", mc.FORWARD_CASES, ids=mc.case_id)
def test_forward_logits_are_not_saturated(case):
    """|z| <= 8 for at least 90 % of a case's rows: sigmoid'(8) = 3.4e-4, so the 1e-4 bar on probabilities still binds the logit there."""
    dim, hidden, n, _, kind = case
    z, p = mc.forward_reference(dim, hidden, n, kind)
    assert z.shape == p.shape == (n,) and np.isfinite(z).all()
    assert (np.abs(z) <= 8).mean() >= 0.9
    assert ((p > 0) & (p < 1)).all()


def test_every_case_takes_the_path_the_table_intends():
    """dygnn_merge_layer_forward_path is host code: the table's intended paths hold on a machine without a GPU too (the GPU module asserts
    the same next to the launches)."""
    from dyglib_amd import _build, _capi
    _build.build(verbose=False)          # hipcc cross-compiles gfx950 without a GPU
    lib = _capi.load()
    got = {(dim, hidden, n): lib.dygnn_merge_layer_forward_path(n, dim, hidden) for dim, hidden, n, _, _ in mc.FORWARD_CASES}
    assert got == {(dim, hidden, n): path for dim, hidden, n, path, _ in mc.FORWARD_CASES}
    assert set(got.values()) == {mc.G, mc.R1, mc.R4, mc.M}
    assert lib.dygnn_merge_layer_forward_path(64, 8200, 4) == -1 and b"dim too large" in lib.dygnn_last_error()
    # sizes near the top of int32 are refused by 64-bit arithmetic, whatever n asks for
    for n in (1, 64, 2048):
        for dim in (2 ** 30, 2 ** 31 - 4, 2 ** 31 - 1):
            assert lib.dygnn_merge_layer_forward_path(n, dim, 4) == -1 and b"dim too large" in lib.dygnn_last_error()
