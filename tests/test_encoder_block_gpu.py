"""The shared TransformerEncoder block (encoder_block_train.h) and row kernels (train_rows.h: k_res_ln<NV> / k_res_ln_bwd<NV> with NV = 4,
5, 8 columns per lane, k_row_drop, the row map) at the widths their templates can get wrong, on an MI355X: training forward and every
parameter gradient with dropout ON (p = 0.1, fixed seed) against the oracles and at the bars of the existing training tests
(tests/parity.py: 1e-4 on embeddings, 1e-4 * max(1, max |ref|) on gradients).  Every case: B = 3, K <= 3, one layer.

  TCL  (NV = 4, row map side -> pair sequence):  node_feat_dim = the largest dygnn_tcl_check accepts (probed, 256: every lane of the last
       slot live) and 236 (no multiple of 64, nor of 16: 44 live lanes in the last slot).  A width that is no multiple of 64 with dropout
       on is also what tests/test_tcl_train_gpu.py::test_dropout_matches_oracle runs on the fixture cases (d = 172); it is not repeated here.
  CAWN (NV = 8, identity map):  attention_dim 312 in (256, 512]: the lane slots beyond 256 columns carry dropped-out elements only here
       (tests/test_cawn_train_gpu.py reaches 260, 312 and 512 at p = 0).
  TGAT (NV = 5, identity map):  query width 264 in (256, 320]: 8 live lanes in the fifth slot.  The library's bound is 272, where
       tests/test_tgat_configs_gpu.py::test_training_against_oracle_autograd[*-dropout] already runs (k1_l3, b1, ft268_h4, ...)."""
import ctypes as C

import numpy as np
import pytest
import torch

from dyglib_amd import _capi
from dyglib_amd import synthetic as syn
from oracle import dygformer_oracle as orc
from oracle import tgat_oracle as torc
from tests import cawn_cases as cc
from tests import tcl_train_oracle as tto
from tests.parity import close, close_scaled

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P_DROP, SEED = 0.1, (3 << 40) + 4711          # the seed's high word reaches the masks (key1)
B, K = 3, 3


def _loss(s, d):
    w = [torch.from_numpy(np.random.RandomState(x).standard_normal(tuple(s.shape)).astype(np.float32)).to(s.device) for x in (1, 2)]
    return (s * w[0]).sum() + (d * w[1]).sum()


def _grads(model):
    return {n: p.grad.detach().cpu().numpy() for n, p in model.named_parameters()}


def _batch(data):
    """the last B interactions; the first root pair moved before every interaction (root-only sequences / empty histories)"""
    E = data.num_interactions
    src, dst, t = data.src_node_ids[E - B:].copy(), data.dst_node_ids[E - B:].copy(), data.node_interact_times[E - B:].copy()
    t[0] = data.node_interact_times.min()
    return src, dst, t


def tcl_widest():
    """the largest node_feat_dim dygnn_tcl_check accepts with two heads, read from the check itself"""
    lib = _capi.load()
    ok = [d for d in range(4, 1025, 4) if lib.dygnn_tcl_check(C.byref(_capi.TclConfig(d, 172, 100, K, 1, 2, 10, 10))) == 0]
    assert ok and ok[-1] < 1024, ok[-3:]
    return ok[-1]


@pytest.mark.parametrize("width", ["widest", 236])
def test_tcl_training_matches_oracle_with_dropout(width):
    from dyglib_amd import get_neighbor_sampler
    from tests.test_tcl_gpu import make_model
    Fn = tcl_widest() if width == "widest" else width
    Fe, Ft, L, H = 172, 100, 1, 2
    data, nf, ef = syn.make_bipartite_graph(60, 15, 1500, seed=71, time_span=2.68e6)
    nf = (np.random.RandomState(72).standard_normal((nf.shape[0], Fn)) * 0.5).astype(np.float32)
    nf[0] = 0.0
    src, dst, t = _batch(data)
    params = syn.make_tcl_params(73, K, num_layers=L, node_feat_dim=Fn, edge_feat_dim=Fe, time_feat_dim=Ft)
    m = make_model(nf, ef, data, params, K, L, H, Ft).train()
    m.dropout, m._fixed_dropout_seed = P_DROP, SEED
    s, d = m.compute_src_dst_node_temporal_embeddings(src, dst, t, num_neighbors=K)
    _loss(s, d).backward()
    got = _grads(m)
    twin = get_neighbor_sampler(data, "recent", seed=1, device=DEV)
    a, b = twin.get_historical_neighbors(src, t, K), twin.get_historical_neighbors(dst, t, K)
    P = {n: torch.from_numpy(v.copy()).requires_grad_(True) for n, v in params.items()}
    os_, od = tto.tcl_train_forward(P, nf, ef, src, dst, t, a, b, L, H, P_DROP, SEED)
    _loss(os_, od).backward()
    tag = f"tcl train d{Fn} p={P_DROP}"
    close(s.detach().cpu().numpy(), os_.detach().numpy(), tag + " src vs oracle", "encoder block: tcl training embeddings with dropout vs oracle")
    close(d.detach().cpu().numpy(), od.detach().numpy(), tag + " dst vs oracle", "encoder block: tcl training embeddings with dropout vs oracle")
    assert set(got) == set(P)
    for n, p in P.items():
        close_scaled(got[n], p.grad.numpy(), f"{tag} grad {n}", label="encoder block: tcl training gradients with dropout vs oracle autograd (scaled bar)")


def test_cawn_training_matches_oracle_with_dropout_past_256_columns():
    from tests.test_cawn_train_gpu import _small_case, compare, hip_sides_run, make_model, oracle_sides_run
    W, Pd, heads = 1, 172, 8
    assert 256 < syn.cawn_attention_dim(172 + 172 + cc.TIME_FEAT_DIM + Pd, heads) <= 512
    c = _small_case(W, K, Pd, heads, B)
    m = make_model(c["data"], c["node_feat"], c["edge_feat"], c["params"], cc.TIME_FEAT_DIM, Pd, W, heads).enable_training()
    got = hip_sides_run(m, c["sides"], K, (1, 2), P_DROP, SEED)
    want = oracle_sides_run(c["params"], c["node_feat"], c["edge_feat"], c["sides"], heads, (1, 2), P_DROP, SEED)
    compare(f"cawn train A312 p={P_DROP}", got, want, "encoder block, dropout past 256 columns")


def test_tgat_training_matches_oracle_with_dropout_past_256_columns():
    from dyglib_amd import TGAT, get_neighbor_sampler
    Fn, Fe, Ft, H, L = 164, 172, 100, 2, 1
    assert 256 < Fn + Ft <= 320
    data, _, ef = syn.make_bipartite_graph(60, 15, 1500, seed=81, time_span=2.68e6, edge_feat_dim=Fe)
    nf = np.random.RandomState(82).standard_normal((data.max_node_id + 1, Fn)).astype(np.float32) * 0.5
    nf[0] = 0.0
    src, dst, t = _batch(data)
    params = syn.make_tgat_params(83, node_feat_dim=Fn, edge_feat_dim=Fe, time_feat_dim=Ft, num_layers=L)
    m = TGAT(nf, ef, get_neighbor_sampler(data, "recent", seed=1, device=DEV), Ft, num_layers=L, num_heads=H, dropout=0.1, device=DEV)
    m.load_state_dict({n: torch.from_numpy(v) for n, v in params.items()}, strict=True)
    m = m.to(DEV).train()
    m.dropout, m._fixed_dropout_seed = P_DROP, SEED
    s, d = m.compute_src_dst_node_temporal_embeddings(src, dst, t, num_neighbors=K)
    _loss(s, d).backward()
    got = _grads(m)
    adj = orc.OracleAdjacency(data.src_node_ids, data.dst_node_ids, data.edge_ids, data.node_interact_times)
    P = {n: torch.from_numpy(v.copy()).requires_grad_(True) for n, v in params.items()}
    both = torc.node_embeddings(P, torch.from_numpy(nf), torch.from_numpy(ef), adj, np.concatenate([src, dst]), np.concatenate([t, t]), L, K, H,
                                dropout=torc.TrainDropout(P_DROP, SEED))
    os_, od = both[:B], both[B:]
    _loss(os_, od).backward()
    tag = f"tgat train Dq{Fn + Ft} p={P_DROP}"
    close(s.detach().cpu().numpy(), os_.detach().numpy(), tag + " src vs oracle", "encoder block: tgat training embeddings with dropout vs oracle")
    close(d.detach().cpu().numpy(), od.detach().numpy(), tag + " dst vs oracle", "encoder block: tgat training embeddings with dropout vs oracle")
    assert set(got) == set(P)
    for n, p in P.items():
        close_scaled(got[n], p.grad.numpy(), f"{tag} grad {n}", label="encoder block: tgat training gradients with dropout vs oracle autograd (scaled bar)")
