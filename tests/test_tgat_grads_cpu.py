"""TGAT parameter gradients: the CPU oracle (oracle/tgat_oracle.py) under torch autograd, parameters as grad-enabled tensors, against
fixtures produced by the REFERENCE TGAT's own autograd (tools/make_golden_tgat_grads.py -> tests/golden/grads_tgat_*.npz; eval mode, so
dropout is the identity).  This pins the oracle the GPU training tests (tests/test_tgat_train_gpu.py) compare with off-fixture.  Bar: that
of tests/test_gradients_golden.py (1e-4 * max(1, max|gradient|))."""
import numpy as np
import pytest
import torch

from oracle import dygformer_oracle as orc
from oracle import tgat_oracle as torc
from tests import golden_cases as gc
from tests.parity import close
from tests.test_gradients_golden import _check

UNIFORM_CASE = "tgat_bip_l2_k20"


def _oracle_grads(c, adj):
    cfg = c["tgat_cfg"]
    params = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in c["tgat_params"].items()}
    nf, ef = torch.from_numpy(c["node_feat"]), torch.from_numpy(c["edge_feat"])
    times = np.asarray(c["times"], dtype=np.float64)
    emb = [torc.node_embeddings(params, nf, ef, adj, ids, times, cfg["num_layers"], cfg["num_neighbors"], cfg["num_heads"])
           for ids in (c["src"], c["dst"])]
    G1, G2 = gc.grad_loss_weights(len(c["src"]))
    loss = (emb[0] * torch.from_numpy(G1)).sum() + (emb[1] * torch.from_numpy(G2)).sum()
    loss.backward()
    return params, loss, emb


def _check_case(name, c, g, adj):
    params, loss, (s, d) = _oracle_grads(c, adj)
    assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-3 * max(1.0, abs(float(g["loss"])))
    close(s.detach().numpy(), g["src_emb"], name + " src")
    close(d.detach().numpy(), g["dst_emb"], name + " dst")
    assert {k for k in g if "|" in k} == {k for k in g if k.split("|")[0] in params and "|" in k}
    _check(name, {k: v.grad.numpy() for k, v in params.items()}, g)


@pytest.mark.parametrize("name", list(gc.TGAT_CASES))
def test_oracle_autograd_matches_reference_tgat_gradients(name):
    c = gc.build_tgat_case(name)
    d = c["data"]
    adj = orc.OracleAdjacency(d.src_node_ids, d.dst_node_ids, d.edge_ids, d.node_interact_times)
    _check_case("grads_" + name, c, gc.load_golden("grads_" + name), adj)


def test_oracle_autograd_matches_reference_tgat_gradients_uniform(monkeypatch):
    """`uniform` sampling: the oracle's recursion draws from the host sampler's RandomState in the reference's order (models/TGAT.py:92-110);
    the gradients of the positive call, then the embeddings of a no_grad negative call on the same sampler."""
    from dyglib_amd import get_neighbor_sampler
    c = gc.build_tgat_case(UNIFORM_CASE)
    g = gc.load_golden("grads_tgat_uniform_" + UNIFORM_CASE)
    strategy, seed, tsf = gc.SAMPLING_STRATEGIES["uniform"]
    sampler = get_neighbor_sampler(c["data"], strategy, time_scaling_factor=tsf, seed=seed, device="cpu")
    d = c["data"]
    adj = orc.OracleAdjacency(d.src_node_ids, d.dst_node_ids, d.edge_ids, d.node_interact_times)

    def draw(_, ids, t, k):
        """utils/utils.py:149-199 on the host: history lengths from the oracle, positions from the sampler's RandomState replay"""
        ids = np.asarray(ids, dtype=np.int64)
        hist = np.array([len(orc.find_neighbors_before(adj, v, tt)[0]) for v, tt in zip(ids, t)], dtype=np.int32)
        sel = sampler._draw_host(ids, hist, k)
        out_n, out_e, out_t = np.zeros((len(ids), k), np.int64), np.zeros((len(ids), k), np.int64), np.zeros((len(ids), k), np.float32)
        for r in np.nonzero(hist > 0)[0]:
            nb, eb, tb = adj.row(int(ids[r]))
            out_n[r], out_e[r], out_t[r] = nb[sel[r]], eb[sel[r]], tb[sel[r]]
        return out_n, out_e, out_t

    monkeypatch.setattr(torc, "get_historical_neighbors_recent", draw)
    _check_case("grads_tgat_uniform", c, g, None)
    cfg = c["tgat_cfg"]
    ns, nd = torc.tgat_forward(c["tgat_params"], c["node_feat"], c["edge_feat"], None, c["src"], c["neg_dst"], c["times"],
                               cfg["num_layers"], cfg["num_neighbors"], cfg["num_heads"])
    close(ns.numpy(), g["neg_src_emb"], "grads_tgat_uniform neg src")
    close(nd.numpy(), g["neg_dst_emb"], "grads_tgat_uniform neg dst")


def test_train_workspace_covers_the_config_range():
    """dygnn_tgat_train_workspace_bytes (no launch): every configuration the inference path takes up to an input row of 1024 floats has a
    training workspace; wider rows and invalid configurations get none (dygnn_tgat_train_forward: DYGNN_E_UNSUPPORTED / _INVALID)."""
    import ctypes as C
    from dyglib_amd import _build, _capi
    _build.build(verbose=False)
    lib = _capi.load()
    ok = _capi.TgatConfig(172, 172, 100, 2, 2, 20)
    assert lib.dygnn_tgat_train_workspace_bytes(C.byref(ok), 200) > lib.dygnn_tgat_workspace_bytes(C.byref(ok), 200) > 0
    for cfg in (_capi.TgatConfig(172, 172, 100, 3, 4, 5), _capi.TgatConfig(172, 172, 100, 1, 2, 64), _capi.TgatConfig(4, 4, 4, 1, 1, 1)):
        assert lib.dygnn_tgat_train_workspace_bytes(C.byref(cfg), 3) > 0
    for cfg in (_capi.TgatConfig(172, 800, 100, 2, 2, 20), _capi.TgatConfig(172, 172, 100, 4, 2, 20), _capi.TgatConfig(172, 172, 100, 2, 2, 65)):
        assert lib.dygnn_tgat_train_workspace_bytes(C.byref(cfg), 3) == 0
