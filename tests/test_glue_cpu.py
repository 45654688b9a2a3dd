"""dyglib_amd/_glue.py, the host glue every backbone calls, without a GPU: input upload, the gradient buffer layout, the parameter snapshot of
a training call, the dropout seed rule, id validation, and the three refusals (CPU model, no backward, parameters that are not float32)."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn as nn

from dyglib_amd import _capi, _glue

CPU = torch.device("cpu")


def _params(sizes=(5, 1, 8, 3)):
    return [nn.Parameter(torch.randn(n)) for n in sizes[:-1]] + [nn.Parameter(torch.randn(sizes[-1], 1))]      # the last one is 2-D


def _starts(views):
    base = min(v.data_ptr() for v in views)
    return [(v.data_ptr() - base) // 4 for v in views]


# ---- to_dev ------------------------------------------------------------------------------------------------------------------------
def test_to_dev_ids_and_times():
    for ids in (np.array([3, 1, 2], dtype=np.int32), torch.tensor([3, 1, 2], dtype=torch.int64)):
        for non_blocking in (False, True):
            out = _glue.to_dev(ids, torch.int64, CPU, non_blocking=non_blocking)
            assert out.dtype == torch.int64 and out.device == CPU and out.is_contiguous() and out.tolist() == [3, 1, 2]
    t32 = np.array([0.5, 1.25, 1e6 + 0.5], dtype=np.float32)
    out = _glue.to_dev(t32, torch.float64, CPU)
    assert out.dtype == torch.float64 and np.array_equal(out.numpy(), t32.astype(np.float64))
    strided = torch.arange(12, dtype=torch.int64).reshape(3, 4).t()
    assert not strided.is_contiguous()
    out = _glue.to_dev(strided, torch.int64, CPU)
    assert out.is_contiguous() and torch.equal(out, strided)


# ---- zero_grads --------------------------------------------------------------------------------------------------------------------
def test_zero_grads_tight_packing():
    params = _params()
    grads = _glue.zero_grads(params, CPU)
    assert [g.shape for g in grads] == [p.shape for p in params]
    assert all(g.dtype == torch.float32 and not g.any() for g in grads)
    assert _starts(grads) == [0, 5, 6, 14]                                               # adjacent slices ...
    assert grads[0].untyped_storage().nbytes() == 4 * 17                                 # ... of one 17-element buffer
    assert len({g.untyped_storage().data_ptr() for g in grads}) == 1


def test_zero_grads_aligned_to_four_floats():
    params = _params()
    grads = _glue.zero_grads(params, CPU, align_floats=4)
    assert [g.shape for g in grads] == [p.shape for p in params] and not any(g.any() for g in grads)
    assert _starts(grads) == [0, 8, 12, 20]
    assert len({g.untyped_storage().data_ptr() for g in grads}) == 1


@pytest.mark.parametrize("align", [1, 4])
def test_zero_grads_views_do_not_overlap(align):
    grads = _glue.zero_grads(_params(), CPU, align_floats=align)
    for i, g in enumerate(grads):
        g.fill_(1.0)
        assert all(not other.any() for j, other in enumerate(grads) if j != i)
        g.zero_()


def test_zero_grads_of_nothing():
    assert _glue.zero_grads([], CPU) == [] and _glue.zero_grads([], CPU, align_floats=4) == []


# ---- param_versions / check_param_versions -----------------------------------------------------------------------------------------
def test_param_versions_pass_when_untouched_and_after_a_data_write():
    params = _params()
    saved = _glue.param_versions(params)
    _glue.check_param_versions(params, saved, "TCL")
    params[1].data.add_(1)                      # today's behaviour: a write through .data bumps no version counter and goes unseen
    _glue.check_param_versions(params, saved, "TCL")


def test_param_versions_see_an_inplace_write():
    params = _params()
    saved = _glue.param_versions(params)
    with torch.no_grad():
        params[2].add_(1)
    with pytest.raises(RuntimeError, match="modified by an inplace operation") as e:
        _glue.check_param_versions(params, saved, "CAWN")
    assert "a CAWN parameter changed between this call's forward and its backward" in str(e.value)


def test_param_versions_see_new_storage():
    params = _params()
    saved = _glue.param_versions(params)
    old = params[0].data                        # kept alive: the new storage cannot land at the old address
    params[0].data = old.clone()
    assert params[0].data_ptr() != old.data_ptr()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        _glue.check_param_versions(params, saved, "TGN")


# ---- dropout_seed ------------------------------------------------------------------------------------------------------------------
def test_dropout_seed_pinned_leaves_the_generator_alone():
    model = nn.Linear(2, 2)
    model._fixed_dropout_seed = 7
    torch.manual_seed(123)
    before = torch.get_rng_state()
    assert _glue.dropout_seed(model) == 7
    assert torch.equal(torch.get_rng_state(), before)


@pytest.mark.parametrize("pin", ["absent", "none"])
def test_dropout_seed_is_one_draw_from_the_generator(pin):
    model = nn.Linear(2, 2)
    if pin == "none":
        model._fixed_dropout_seed = None                   # how the tests un-pin it
    torch.manual_seed(123)
    want = int(torch.randint(0, 2 ** 62, (1,)).item())
    state_after_one_draw = torch.get_rng_state()
    torch.manual_seed(123)
    assert _glue.dropout_seed(model) == want
    assert torch.equal(torch.get_rng_state(), state_after_one_draw)


# ---- validate_ids ------------------------------------------------------------------------------------------------------------------
class _CountingCsr:
    def __init__(self):
        self.tables, self.queries = [], []

    def check_tables(self, node_rows, edge_rows):
        self.tables.append((node_rows, edge_rows))

    def check_query_ids(self, ids, limit):
        self.queries.append((ids, limit))


def test_validate_ids_checks_tables_once_per_csr_and_ids_every_call():
    class Model:
        pass
    model, a, b = Model(), _CountingCsr(), _CountingCsr()
    src, dst = np.array([1, 2]), np.array([3, 4])
    _glue.validate_ids(model, a, (src, dst), 90, 100, 2000)
    _glue.validate_ids(model, a, (src, dst), 90, 100, 2000)
    assert a.tables == [(100, 2000)]
    assert [(ids is arr, limit) for (ids, limit), arr in zip(a.queries, (src, dst, src, dst))] == [(True, 90)] * 4
    assert model._validated_csr is a
    _glue.validate_ids(model, b, (src,), 7, 8, 9)
    assert b.tables == [(8, 9)] and len(b.queries) == 1 and b.queries[0][1] == 7 and model._validated_csr is b
    _glue.validate_ids(model, a, (), 90, 100, 2000)                # back to the first sampler: its graph is checked again
    assert a.tables == [(100, 2000)] * 2 and len(a.queries) == 4


# ---- the refusals ------------------------------------------------------------------------------------------------------------------
def test_require_cuda_tables_refuses_a_cpu_model():
    class Backbone:
        node_raw_features = edge_raw_features = torch.zeros(1, 1)
    with pytest.raises(_capi.DygnnError) as e:
        _glue.require_cuda_tables(Backbone(), CPU)
    assert str(e.value) == "dyglib_amd.Backbone runs on an MI355X only; there is no CPU fallback"


def test_refuse_untrainable_truth_table():
    """Against the expression as the backbones spelled it before they shared it.  Its three inputs are (grad enabled; training or any
    requires_grad; trainable and training); the third implies the second, which leaves six of the eight rows reachable: all six are seen."""
    seen = set()
    for grad, training, requires_grad, trainable in itertools.product((False, True), repeat=4):
        model = nn.Linear(2, 2).train(training)
        for p in model.parameters():
            p.requires_grad_(requires_grad)
        with torch.set_grad_enabled(grad):
            want = (torch.is_grad_enabled() and (model.training or any(p.requires_grad for p in model.parameters()))
                    and not (trainable and model.training))
            seen.add((grad, training or requires_grad, trainable and training))
            if want:
                with pytest.raises(NotImplementedError, match="^the caller's message$"):
                    _glue.refuse_untrainable(model, trainable, "the caller's message")
            else:
                _glue.refuse_untrainable(model, trainable, "the caller's message")
    assert seen == {(g, b, c) for g in (False, True) for b, c in ((False, False), (True, False), (True, True))}


def test_require_f32_params():
    _glue.require_f32_params(_params())
    for bad in (nn.Parameter(torch.zeros(3, dtype=torch.float64)), nn.Parameter(torch.zeros(3, 4).t())):
        with pytest.raises(_capi.DygnnError) as e:
            _glue.require_f32_params(_params() + [bad])
        assert str(e.value) == "parameters must be contiguous float32"
