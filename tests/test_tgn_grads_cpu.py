"""TGN parameter gradients: the test-side autograd composition of the CPU oracle (tests/tgn_autograd.py) against fixtures produced by the
REFERENCE MemoryModel('TGN')'s own autograd (tools/make_golden_tgn_grads.py -> tests/golden/grads_tgn_*.npz; eval mode, so dropout is the
identity; every batch but the last replayed under no_grad, the last batch's negative and positive call differentiated).  This pins the
composition the GPU training tests (tests/test_tgn_train_gpu.py) compare with off-fixture.  Bars: those of tests/test_tgat_grads_cpu.py
(loss 1e-3 * max(1, |loss|); embeddings and memories 1e-4; gradients 1e-4 * max(1, max|gradient|) through _check)."""
import ctypes as C

import numpy as np
import pytest

from oracle import tgn_oracle as norc
from tests import golden_cases as gc
from tests import tgn_autograd as ta
from tests.parity import close
from tests.test_gradients_golden import _check


def _check_case(name, c, g, adj=None):
    params, loss, embs, st = ta.last_batch_grads(c, adj)
    assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-3 * max(1.0, abs(float(g["loss"])))
    for key, e in zip(("neg_src_emb", "neg_dst_emb", "pos_src_emb", "pos_dst_emb"), embs):
        close(e.detach().numpy(), g[key], f"{name} {key}")
    close(st.M.numpy(), g["final_memory"], name + " final memory")
    close(st.U.numpy(), g["final_last_update"], name + " final last update")
    got = {k: v.grad.numpy() for k, v in params.items() if v.grad is not None}
    assert sorted(got) == g["params_with_grad"].tolist()
    assert {k.split("|")[0] for k in g if "|" in k} == set(got)
    assert not any("memory_bank" in k for k in got)
    gru = "memory_updater.memory_updater."
    assert np.abs(got[gru + "weight_ih"]).max() > 0 and np.abs(got[gru + "weight_hh"]).max() > 0
    _check(name, got, g)


@pytest.mark.parametrize("name", list(gc.TGN_CASES))
def test_oracle_autograd_matches_reference_tgn_gradients(name):
    _check_case("grads_" + name, gc.build_tgn_case(name), gc.load_golden("grads_" + name))


def test_oracle_autograd_matches_reference_tgn_gradients_uniform(monkeypatch):
    """`uniform` sampling from the first batch on: the oracle's recursion draws from the host sampler's RandomState in the reference's order
    (one draw on [src ; dst] per call, MemoryModel.py:104-131, :626-629)."""
    from dyglib_amd import get_neighbor_sampler
    c = gc.build_tgn_case(ta.UNIFORM_CASE)
    strategy, seed, tsf = gc.SAMPLING_STRATEGIES["uniform"]
    sampler = get_neighbor_sampler(c["data"], strategy, time_scaling_factor=tsf, seed=seed, device="cpu")
    adj = ta.adjacency(c["data"])
    monkeypatch.setattr(norc, "get_historical_neighbors_recent", ta.uniform_draw(sampler, adj))
    _check_case("grads_tgn_uniform", c, gc.load_golden("grads_tgn_uniform_" + ta.UNIFORM_CASE), adj)


def test_train_workspace_covers_the_config_range():
    """dygnn_tgn_train_workspace_bytes (no launch): BASELINE config 5 and the corner configurations both dygnn_tgn_forward_step and
    dygnn_tgat_train_forward take have a training workspace, larger than the inference one; wider rows, more layers or neighbours, no nodes
    and an empty batch get none (dygnn_tgn_train_forward: DYGNN_E_UNSUPPORTED / _INVALID).  The sizes are compared at BASELINE's batch of 200
    pairs: the training call keeps every activation of every level entry, which grows with the batch, while the inference workspace starts
    from a per-call packed copy of the layer weights (2 MB per layer) that the training path does not make, so at a batch of a few pairs
    the comparison would measure that copy and not the activations."""
    from dyglib_amd import _build, _capi
    _build.build(verbose=False)
    lib = _capi.load()
    N = 7145
    ok = _capi.TgatConfig(172, 172, 100, 1, 2, 10)                    # BASELINE config 5
    assert lib.dygnn_tgn_train_workspace_bytes(C.byref(ok), N, 200) > lib.dygnn_tgn_workspace_bytes(C.byref(ok), N, 200) > 0
    for cfg in (_capi.TgatConfig(172, 172, 100, 3, 4, 5), _capi.TgatConfig(172, 172, 100, 1, 2, 64), _capi.TgatConfig(172, 172, 100, 2, 4, 4),
                _capi.TgatConfig(4, 4, 4, 1, 1, 1)):
        assert lib.dygnn_tgn_train_workspace_bytes(C.byref(cfg), N, 200) > lib.dygnn_tgn_workspace_bytes(C.byref(cfg), N, 200) > 0
        assert lib.dygnn_tgn_train_workspace_bytes(C.byref(cfg), 50, 3) > 0
    for cfg in (_capi.TgatConfig(172, 800, 100, 2, 2, 20), _capi.TgatConfig(172, 172, 100, 4, 2, 20), _capi.TgatConfig(172, 172, 100, 2, 2, 65),
                _capi.TgatConfig(172, 172, 100, 1, 3, 10)):
        assert lib.dygnn_tgn_train_workspace_bytes(C.byref(cfg), 50, 3) == 0
    assert lib.dygnn_tgn_train_workspace_bytes(C.byref(ok), 0, 3) == 0
    assert lib.dygnn_tgn_train_workspace_bytes(C.byref(ok), N, 0) == 0
