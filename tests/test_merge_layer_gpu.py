"""The link-predictor head on every kernel it dispatches to (dygnn_merge_layer_sigmoid / _logits / _backward, dyglib_amd/csrc/merge_layer.hip,
behind dyglib_amd.modules.MergeLayer) against the float64 reference of tests/merge_layer_cases.py.

Forward: the four kernels G / R1 / R4 / M at the widths and ragged row counts of the case table, logits and probabilities within the project's
forward bar (tests.parity.close, 1e-4 absolute; one label per path).  Tolerance-free properties: nothing is written outside out[0, n), a
permutation of the rows permutes the outputs bit for bit, a NaN row gives NaN and changes no other row.  Backward: input gradients within the
same bar, parameter gradients within the scaled bar, into buffers pre-filled so that "writes" and "accumulates" are both visible."""
import functools

import numpy as np
import pytest
import torch

from dyglib_amd import MergeLayer, _capi
from tests import merge_layer_cases as mc
from tests.parity import close, close_scaled

pytestmark = pytest.mark.gpu
PAD = 64                                   # sentinel elements behind out[n]
SENTINEL_BITS = 0x7FC5A5A5             # a quiet NaN with a payload no kernel produces
PAD_ROWS = 16                              # sentinel rows behind grad_a / grad_b


def _sentinel(*shape):
    return torch.full(shape, SENTINEL_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


def _untouched(t):
    return bool((t.contiguous().view(torch.int32) == SENTINEL_BITS).all())


def _cuda(x):
    return torch.from_numpy(np.array(x)).cuda()


@functools.lru_cache(maxsize=None)
def dev_params(dim, hidden, kind="nn"):
    return {k: _cuda(v) for k, v in mc.params(dim, hidden, kind).items()}


def forward(which, a, b, P):
    """One library call on device tensors a, b [n, dim]; returns out [n].  The 64 elements behind it must come back as they were."""
    lib = _capi.load()
    n, dim = a.shape
    hidden = P["fc1.weight"].shape[0]
    assert a.is_contiguous() and b.is_contiguous() and b.shape == a.shape and P["fc1.weight"].shape == (hidden, 2 * dim)
    buf = _sentinel(n + PAD)
    fn = {"logits": lib.dygnn_merge_layer_logits, "sigmoid": lib.dygnn_merge_layer_sigmoid}[which]
    _capi.check(fn(a.data_ptr(), b.data_ptr(), n, dim, hidden, P["fc1.weight"].data_ptr(), P["fc1.bias"].data_ptr(), P["fc2.weight"].data_ptr(),
                   P["fc2.bias"].data_ptr(), buf.data_ptr(), _capi.current_stream_ptr()))
    torch.cuda.synchronize()
    assert _untouched(buf[n:]), f"{which}: wrote behind out[{n}]"
    return buf[:n]


def forward_case(which, dim, hidden, n, kind="nn"):
    a, b = mc.forward_inputs(dim, hidden, n)
    return forward(which, _cuda(a), _cuda(b), dev_params(dim, hidden, kind))


def path_of(n, dim, hidden):
    return _capi.load().dygnn_merge_layer_forward_path(n, dim, hidden)


# ---- paths ---------------------------------------------------------------------------------------------------------------------------------
def test_every_case_takes_the_path_the_table_intends_and_all_four_are_taken():
    taken = set()
    for dim, hidden, n, want, _ in mc.FORWARD_CASES:
        got = path_of(n, dim, hidden)
        assert got == want, (dim, hidden, n, mc.PATH_NAMES.get(got, got), mc.PATH_NAMES[want])
        taken.add(got)
    assert taken == {mc.G, mc.R1, mc.R4, mc.M}
    for dim, hidden, n, want in mc.ONE_PER_PATH:
        assert path_of(n, dim, hidden) == want
    # a single row of dim 8200 needs 2 * 8200 + 4 floats of LDS, more than 64 KB: refused with the library's error code wherever the one-row
    # kernel is all that is left (from 2048 rows on a dim that is a multiple of 4 has the wave-per-16-rows kernel, which stages nothing)
    for n, dim in ((1, 8200), (64, 8200), (2047, 8200), (2048, 8202)):
        rc = path_of(n, dim, 4)
        assert rc == -1
        with pytest.raises(AssertionError, match="dim too large"):
            _capi.check(rc)
    assert path_of(2048, 8200, 4) == mc.M
    assert path_of(5, 0, 4) == -1 and path_of(-1, 4, 4) == -1 and path_of(5, 4, 0) == -1


# ---- forward against the reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.FORWARD_CASES, ids=mc.case_id)
def test_forward_matches_the_float64_reference(case):
    dim, hidden, n, path, kind = case
    assert path_of(n, dim, hidden) == path
    z, p = mc.forward_reference(dim, hidden, n, kind)
    name = mc.PATH_NAMES[path]
    close(forward_case("logits", dim, hidden, n, kind).cpu().numpy(), z, f"merge head logits {mc.case_id(case)}", label=f"merge head logits, path {name}")
    close(forward_case("sigmoid", dim, hidden, n, kind).cpu().numpy(), p, f"merge head probabilities {mc.case_id(case)}",
          label=f"merge head probabilities, path {name}")


RAGGED = [(path, n) for path in (mc.G, mc.R1, mc.R4, mc.M) for n in mc.RAGGED_N[path]]


@pytest.mark.parametrize("path,n", RAGGED, ids=[f"{mc.PATH_NAMES[path]}-n{n}" for path, n in RAGGED])
def test_forward_writes_rows_0_to_n_and_nothing_else(path, n):
    """out has 64 sentinel elements behind row n (a NaN bit pattern): every one of them survives (checked inside forward()), and every row
    below n was written (none keeps the sentinel) — at the row counts where the last workgroup / wave of each kernel is ragged."""
    dim, hidden = (172, 260) if path == mc.M else (172, 172)
    assert path_of(n, dim, hidden) == path
    for which in ("logits", "sigmoid"):
        out = forward_case(which, dim, hidden, n)
        assert out.shape == (n,) and bool(torch.isfinite(out).all())


# ---- tolerance-free properties -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.ONE_PER_PATH, ids=mc.case_id)
@pytest.mark.parametrize("which", ["logits", "sigmoid"])
def test_permuting_the_rows_permutes_the_outputs_bit_for_bit(case, which):
    """A row's result depends on no other row of the call and on no position inside a workgroup, an MFMA tile or an LDS stage; the same call
    twice gives the same bits."""
    dim, hidden, n, path = case
    assert path_of(n, dim, hidden) == path
    a, b = (_cuda(x) for x in mc.forward_inputs(dim, hidden, n))
    P = dev_params(dim, hidden)
    out = forward(which, a, b, P)
    assert torch.equal(forward(which, a, b, P), out)
    for seed in (0, 1):
        perm = torch.from_numpy(np.random.RandomState(seed).permutation(n)).cuda()
        assert torch.equal(forward(which, a[perm].contiguous(), b[perm].contiguous(), P), out[perm]), seed
    rev = torch.arange(n - 1, -1, -1, device="cuda")
    assert torch.equal(forward(which, a[rev].contiguous(), b[rev].contiguous(), P), out[rev])


@pytest.mark.parametrize("case", mc.ONE_PER_PATH, ids=mc.case_id)
def test_a_nan_row_gives_nan_and_leaves_every_other_row_alone(case):
    """torch.relu(nan) is nan (models/modules.py:66): a row of NaN embeddings must come out as NaN, not as sigmoid(fc2.bias)."""
    dim, hidden, n, path = case
    a, b = (_cuda(x) for x in mc.forward_inputs(dim, hidden, n))
    P = dev_params(dim, hidden)
    for r in sorted({0, n // 2 + 1, n - 1}):
        bad = a.clone()
        bad[r] = float("nan")
        for which in ("logits", "sigmoid"):
            clean, got = forward(which, a, b, P), forward(which, bad, b, P)
            assert bool(torch.isnan(got[r])), (which, r, float(got[r]))
            keep = torch.ones(n, dtype=torch.bool, device="cuda")
            keep[r] = False
            assert torch.equal(got[keep], clean[keep]), (which, r)
    # ... in the second operand and in a single feature as well
    bad = b.clone()
    bad[n // 2, dim - 1] = float("nan")
    got = forward("sigmoid", a, bad, P)
    assert bool(torch.isnan(got[n // 2])) and int(torch.isnan(got).sum()) == 1


# ---- rows too long for a row block's LDS stage ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,n_lo,n_hi", mc.LONG_ROW_PAIRS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"n{v}")
def test_a_width_answered_below_a_threshold_is_answered_above_it(width, n_lo, n_hi):
    """(516, 4): 16 staged rows exceed 64 KB of LDS, so n = 2048 takes the 4-row form as n = 2047 does; (4100, 4): 4 rows exceed it, so n = 64
    takes the one-row kernel as n = 63 does, and n = 2048 the wave-per-16-rows kernel.  Both n return DYGNN_OK, match the reference and agree
    on their common rows."""
    dim, hidden = width
    for which, ref_i in (("logits", 0), ("sigmoid", 1)):
        lo, hi = forward_case(which, dim, hidden, n_lo).cpu().numpy(), forward_case(which, dim, hidden, n_hi).cpu().numpy()
        close(lo, mc.forward_reference(dim, hidden, n_lo)[ref_i], f"merge head {which} {width} n={n_lo}", label="merge head, long rows vs reference")
        close(hi, mc.forward_reference(dim, hidden, n_hi)[ref_i], f"merge head {which} {width} n={n_hi}", label="merge head, long rows vs reference")
        close(hi[:n_lo], lo, f"merge head {which} {width} n={n_hi} vs n={n_lo}", label="merge head, long rows: common rows of the two n")


# ---- the module reaches the same kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.ONE_PER_PATH[:3], ids=mc.case_id)
def test_the_module_returns_what_the_library_returns(case):
    dim, hidden, n, _ = case
    m = MergeLayer(dim, dim, hidden, 1)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in mc.params(dim, hidden).items()})
    m = m.cuda()
    a, b = (_cuda(x) for x in mc.forward_inputs(dim, hidden, n))
    assert torch.equal(m.link_probabilities(a, b), forward_case("sigmoid", dim, hidden, n))
    with torch.no_grad():
        z = m(a, b)
    assert z.shape == (n, 1) and torch.equal(z[:, 0], forward_case("logits", dim, hidden, n))


# ---- backward ----------------------------------------------------------------------------------------------------------------------------------
def _pattern(numel):
    return (0.25 * (torch.arange(numel, device="cuda") % 7 + 1)).float()            # 0.25 .. 1.75, exact in float32, nowhere zero


def backward(dim, hidden, n, kind="nn", ws_offset=0, inputs=None):
    """dygnn_merge_layer_backward on a backward case.  grad_a / grad_b arrive filled with the sentinel and 16 rows too long, the workspace 64
    floats too long, the four parameter gradients filled with a pattern; returns everything as it comes back."""
    lib = _capi.load()
    a, b, g = (_cuda(x) for x in (inputs or mc.backward_inputs(dim, hidden, n, kind)))
    P = dev_params(dim, hidden, kind)
    da, db = _sentinel(n + PAD_ROWS, dim), _sentinel(n + PAD_ROWS, dim)
    ws = _sentinel(n * hidden + PAD)
    sizes = [hidden * 2 * dim, hidden, hidden, 1]
    grads = [_pattern(s) for s in sizes]
    rc = lib.dygnn_merge_layer_backward(a.data_ptr(), b.data_ptr(), n, dim, hidden, P["fc1.weight"].data_ptr(), P["fc1.bias"].data_ptr(),
                                        P["fc2.weight"].data_ptr(), g.data_ptr(), da.data_ptr(), db.data_ptr(), *(t.data_ptr() for t in grads),
                                        ws.data_ptr() + ws_offset, _capi.current_stream_ptr())
    torch.cuda.synchronize()
    return rc, da, db, grads, ws


@pytest.mark.parametrize("case", mc.BACKWARD_CASES, ids=mc.case_id)
def test_backward_matches_float64_autograd(case):
    dim, hidden, n, kind = case
    ref = mc.backward_reference(*case)
    rc, da, db, grads, ws = backward(dim, hidden, n, kind)
    _capi.check(rc)
    # input gradients: rows [0, n) written (finite: close() asserts it, the buffers held NaN), the 16 rows behind them untouched
    close(da[:n].cpu().numpy(), ref["a"], f"merge backward grad_a {mc.case_id(case)}", label="merge head backward, input gradients")
    close(db[:n].cpu().numpy(), ref["b"], f"merge backward grad_b {mc.case_id(case)}", label="merge head backward, input gradients")
    assert _untouched(da[n:]) and _untouched(db[n:]) and _untouched(ws[n * hidden:])
    # parameter gradients: ACCUMULATED into what the buffers held
    for got, key in zip(grads, ("w1", "b1", "w2", "b2")):
        want = ref[key].reshape(-1)
        added = got.cpu().numpy().astype(np.float64) - _pattern(got.numel()).cpu().numpy().astype(np.float64)
        close_scaled(added, want, f"merge backward grad {key} {mc.case_id(case)}", label="merge head backward, parameter gradients (scaled bar)")


def test_the_forward_of_a_backward_case_matches_too():
    """The logits the training step's forward returns for the inputs of the backward cases (n = 130: path R1; the small n: path G)."""
    for dim, hidden, n, kind in mc.BACKWARD_CASES:
        if n not in (17, 130):
            continue
        a, b, _ = mc.backward_inputs(dim, hidden, n, kind)
        got = forward("logits", _cuda(a), _cuda(b), dev_params(dim, hidden, kind))
        close(got.cpu().numpy(), mc.backward_reference(dim, hidden, n, kind)["z"], f"merge logits of backward case d{dim}h{hidden}n{n}",
              label="merge head logits, inputs of the backward cases")


@pytest.mark.parametrize("dim,hidden,ws_offset,message", [
    (172, 196, 0, "hidden <= 192"), (172, 170, 0, "multiples of 4"), (170, 172, 0, "multiples of 4"), (172, 172, 4, "16-byte aligned")],
    ids=["hidden196", "hidden170", "dim170", "workspace+4"])
def test_backward_refuses_what_it_cannot_run(dim, hidden, ws_offset, message):
    """Sizes outside the backward's contract and a misaligned workspace are the library's error with its message; nothing is launched: every
    output buffer comes back as it went in."""
    n = 33
    rs = np.random.RandomState(5)
    inputs = rs.standard_normal((n, dim)).astype(np.float32), rs.standard_normal((n, dim)).astype(np.float32), rs.standard_normal(n).astype(np.float32)
    rc, da, db, grads, ws = backward(dim, hidden, n, ws_offset=ws_offset, inputs=inputs)
    assert rc == -1
    with pytest.raises(AssertionError, match=message):
        _capi.check(rc)
    assert _untouched(da) and _untouched(db) and _untouched(ws)
    for t in grads:
        assert torch.equal(t, _pattern(t.numel()))


def test_merge_layer_with_a_dim_outside_the_library_range_trains_through_pytorch():
    """dim % 4 != 0 is outside the library's backward (float4 rows): the module must take the PyTorch ops in both directions, as it does for
    a hidden size outside the range, and train."""
    dim, hidden, n = 170, 172, 33
    torch.manual_seed(4)
    ref = MergeLayer(dim, dim, hidden, 1).double()
    hip = MergeLayer(dim, dim, hidden, 1)
    hip.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    hip = hip.cuda()
    a, b = torch.randn(n, dim), torch.randn(n, dim)
    y = (torch.arange(n) % 2).double()
    loss_of = lambda z: torch.nn.functional.binary_cross_entropy_with_logits(z[:, 0], y.to(z.device, z.dtype))
    ar, br = a.double().requires_grad_(True), b.double().requires_grad_(True)
    zr = ref(ar, br)
    loss_of(zr).backward()
    ah, bh = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    z = hip(ah, bh)
    assert "Merge" not in type(z.grad_fn).__name__                     # not the library's autograd function
    close(z.detach().cpu().numpy(), zr.detach().numpy(), "merge dim=170 logits", label="MergeLayer (PyTorch path) logits")
    loss = loss_of(z)
    loss.backward()                                                     # must not raise
    close(ah.grad.cpu().numpy(), ar.grad.numpy(), "merge dim=170 d input_1", label="MergeLayer (PyTorch path) input gradients")
    close(bh.grad.cpu().numpy(), br.grad.numpy(), "merge dim=170 d input_2", label="MergeLayer (PyTorch path) input gradients")
    for (k, ph), (_, pr) in zip(hip.named_parameters(), ref.named_parameters()):
        close_scaled(ph.grad.cpu().numpy(), pr.grad.numpy(), f"merge dim=170 grad {k}", label="MergeLayer (PyTorch path) parameter gradients")
    opt = torch.optim.SGD(hip.parameters(), lr=0.1)
    opt.step()
    with torch.no_grad():
        assert float(loss_of(hip(ah, bh))) < float(loss)
    # the evaluation head is forward only and takes any dim: the one-row kernel
    assert path_of(n, dim, hidden) == mc.G
    with torch.no_grad():
        want = torch.sigmoid(hip(ah, bh))[:, 0]
    close(hip.link_probabilities(ah.detach(), bh.detach()).cpu().numpy(), want.cpu().numpy(), "merge dim=170 link_probabilities",
          label="merge head probabilities, path G")
