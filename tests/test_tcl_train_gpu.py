"""TCL training on the HIP path (dygnn_tcl_train_forward / dygnn_tcl_backward, dyglib_amd/csrc/tcl_train.hip, through _TclTrainFunction)
on an MI355X: against the reference's own autograd (tests/golden/grads_tcl_<case>.npz) at p = 0, against the differentiable restatement
(tests/tcl_train_oracle.py, pinned to the same fixtures by tests/test_tcl_grads_cpu.py) at shapes that have no fixture and with dropout,
plus the autograd plumbing (two calls before one backward, guards, empty batches) and short training runs.  Bars: tests/parity.py, plain
1e-4 on forward quantities, 1e-4 * max(1, max |ref|) on gradients (weight gradients are atomic sums: never compared for equality)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dyglib_amd import synthetic as syn
from tests import golden_cases as gc
from tests import tcl_cases as tc
from tests import tcl_train_oracle as tto
from tests.parity import close, close_scaled
from tests.test_gradients_golden import _check
from tests.test_tcl_gpu import DEV, case_model, make_model
from tests.test_tcl_grads_cpu import oracle_grads
from tests.test_tcl_oracle_golden import OracleSampler

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grads(model):
    return {n: (None if p.grad is None else p.grad.detach().cpu().numpy()) for n, p in model.named_parameters()}


def _fixture_loss(s, d):
    G1, G2 = gc.grad_loss_weights(s.shape[0])
    return (s * torch.from_numpy(G1).to(s.device)).sum() + (d * torch.from_numpy(G2).to(d.device)).sum()


def _train_case(name, p=0.0, seed=None):
    c, cfg, m = case_model(name)
    m.train()
    m.dropout = p
    if seed is not None:
        m._fixed_dropout_seed = seed
    m.set_neighbor_sampler(m.neighbor_sampler)
    return c, cfg, m


# ---- 1. the reference's own gradients --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tc.CASES))
def test_gradients_match_reference_autograd(name):
    c, cfg, m = _train_case(name)
    g = gc.load_golden(f"grads_tcl_{name}")
    s, d = m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=cfg["K"])
    assert s.requires_grad and d.requires_grad
    close(s.detach().cpu().numpy(), g["src_emb"], f"{name} train src_emb", "tcl training embeddings vs reference")
    close(d.detach().cpu().numpy(), g["dst_emb"], f"{name} train dst_emb", "tcl training embeddings vs reference")
    _fixture_loss(s, d).backward()
    grads = _grads(m)
    assert all(v is not None for v in grads.values()) and set(grads) == set(c["tcl_params"])
    _check(f"tcl hip {name}", grads, g)
    if cfg["strategy"] != "recent":                       # the RandomState was consumed as by the reference's call
        with torch.no_grad():
            sn, nd = m.compute_src_dst_node_temporal_embeddings(c["src"], c["neg_dst"], c["times"], num_neighbors=cfg["K"])
        close(sn.cpu().numpy(), g["src_neg_emb"], f"{name} src_neg_emb after the training call", "tcl training embeddings vs reference")
        close(nd.cpu().numpy(), g["neg_dst_emb"], f"{name} neg_dst_emb after the training call", "tcl training embeddings vs reference")


# ---- 2. shapes without a fixture, against the restatement's autograd -----------------------------------------------------------------------------
def _offfixture_case(K, L, H, B, dims, seed):
    """test_tgat_train_gpu._offfixture_case for TCL: a bipartite graph with non-zero node features; the batch = the last interactions, the
    first three roots moved before every interaction (root-only sequences: every neighbour slot padded)"""
    Fn, Fe, Ft = dims
    data, nf, ef = syn.make_bipartite_graph(60, 15, 1500, seed=seed, time_span=2.68e6)
    nf = (np.random.RandomState(seed + 1).standard_normal((nf.shape[0], Fn)) * 0.5).astype(np.float32)
    nf[0] = 0.0
    ef = np.ascontiguousarray(ef[:, :Fe])
    E = data.num_interactions
    src, dst, t = data.src_node_ids[E - B:].copy(), data.dst_node_ids[E - B:].copy(), data.node_interact_times[E - B:].copy()
    t[:3] = data.node_interact_times.min()
    params = syn.make_tcl_params(seed + 2, K, num_layers=L, node_feat_dim=Fn, edge_feat_dim=Fe, time_feat_dim=Ft)
    return dict(data=data, node_feat=nf, edge_feat=ef, src=src, dst=dst, times=t, params=params, Ft=Ft)


def _loss(s, d, seeds, rows=None):
    B, F = s.shape
    w = [torch.from_numpy(np.random.RandomState(x).standard_normal((B, F)).astype(np.float32)).to(s.device) for x in seeds]
    if rows is not None:
        for x in w:
            x[rows:] = 0.0
    return (s * w[0]).sum() + (d * w[1]).sum()


SHAPES = [  # K, L, H, B, (Fn, Fe, Ft)
    (63, 1, 2, 3, (172, 172, 100)),      # S = 64: four full row tiles
    (1, 2, 2, 1, (172, 172, 100)),       # S = 2, one pair
    (16, 3, 4, 7, (172, 172, 100)),      # head dim 43, S one past a tile, 14 * 17 rows: no multiple of 64
    (7, 2, 2, 9, (40, 24, 24)),          # dims that are no multiples of 16
]


@pytest.mark.parametrize("K,L,H,B,dims", SHAPES, ids=[f"K{s[0]}-L{s[1]}-H{s[2]}-B{s[3]}-d{s[4][0]}" for s in SHAPES])
def test_gradients_match_oracle_autograd(K, L, H, B, dims):
    from dyglib_amd import get_neighbor_sampler
    from dyglib_amd.tcl import _TclTrainFunction
    c = _offfixture_case(K, L, H, B, dims, seed=60 + K)
    m = make_model(c["node_feat"], c["edge_feat"], c["data"], c["params"], K, L, H, c["Ft"]).train()
    m.dropout = 0.0
    s, d = m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=K)
    _loss(s, d, (1, 2)).backward()
    got = _grads(m)
    twin = get_neighbor_sampler(c["data"], "recent", seed=1, device=DEV)
    a, b = twin.get_historical_neighbors(c["src"], c["times"], K), twin.get_historical_neighbors(c["dst"], c["times"], K)
    assert not a[0][:min(3, B)].any() and not b[0][:min(3, B)].any()                  # the root-only sequences are there
    P = {n: torch.from_numpy(v.copy()).requires_grad_(True) for n, v in c["params"].items()}
    os_, od = tto.tcl_train_forward(P, c["node_feat"], c["edge_feat"], c["src"], c["dst"], c["times"], a, b, L, H)
    tag = f"tcl train K{K} L{L} H{H} B{B} d{dims[0]}"
    close(s.detach().cpu().numpy(), os_.detach().numpy(), tag + " src vs oracle", "tcl training embeddings vs oracle")
    close(d.detach().cpu().numpy(), od.detach().numpy(), tag + " dst vs oracle", "tcl training embeddings vs oracle")
    _loss(os_, od, (1, 2)).backward()
    assert set(got) == set(P)
    for n, p in P.items():
        ref = p.grad.numpy()
        assert got[n] is not None, n
        close_scaled(got[n], ref, f"{tag} grad {n}", label="tcl training gradients vs oracle autograd (scaled bar)")
        if n.endswith("bias") or "norm_layers" in n:
            g_, r_ = got[n], ref
            if n.endswith("in_proj_bias"):
                # The KEY third of in_proj_bias has a gradient that is zero in exact arithmetic (a constant added to every key of a row
                # leaves its softmax unchanged: sum_j dS_ij = 0), so both sides hold rounding residue there and which elements round to
                # exactly 0.0 is noise.  The residue itself is held to the bar above; the zero pattern is checked on the query and value thirds.
                F = dims[0]
                assert np.abs(r_[F:2 * F]).max() <= 1e-4 * max(1.0, np.abs(r_).max()) and np.abs(g_[F:2 * F]).max() <= 1e-4 * max(1.0, np.abs(r_).max())
                g_, r_ = np.delete(g_, np.s_[F:2 * F]), np.delete(r_, np.s_[F:2 * F])
            bad = np.flatnonzero((g_ != 0) != (r_ != 0))
            assert bad.size == 0, (n, bad[:8].tolist(), g_[bad[:8]].tolist(), r_[bad[:8]].tolist())
    if K != 16:
        return
    # padded positions: a loss that reads ONLY the first pair (root-only sequences: all K slots padded), once as sampled and once with other
    # edge ids and times in every padded slot of the call (the ids stay 0: that is what makes a slot padded).  Padded positions are reachable
    # only as masked keys, so neither the embeddings nor any gradient may move.
    runs = []
    for poke in (False, True):
        m.zero_grad(set_to_none=True)
        (src, dst), tms = m._inputs((c["src"], c["dst"]), c["times"], K, trainable=True)
        roots, tt, nbr, eid, nts = m._sample([src, dst], tms, K)
        if poke:
            pad = nbr == 0
            assert bool(pad[0].all()) and bool(pad[B].all()) and int(pad.sum()) > 2 * K
            rs = np.random.RandomState(5)
            eid = torch.where(pad, torch.from_numpy(rs.randint(1, c["edge_feat"].shape[0], tuple(eid.shape))).to(eid), eid)
            nts = torch.where(pad, torch.from_numpy(rs.uniform(0, 2.68e6, tuple(nts.shape)).astype(np.float32)).to(nts), nts)
        s1, d1 = _TclTrainFunction.apply(m, (roots, tt, nbr, eid.contiguous(), nts.contiguous()), B, K, 0.0, 0, *m.parameters())
        _loss(s1, d1, (3, 4), rows=1).backward()
        runs.append((s1.detach().cpu().numpy(), d1.detach().cpu().numpy(), _grads(m)))
    close(runs[1][0][:1], runs[0][0][:1], tag + " padded slots poked: src", "tcl training: padded slots do not reach the first pair")
    close(runs[1][1][:1], runs[0][1][:1], tag + " padded slots poked: dst", "tcl training: padded slots do not reach the first pair")
    assert any(np.abs(v).max() > 0 for v in runs[0][2].values())
    for n in runs[0][2]:
        close_scaled(runs[1][2][n], runs[0][2][n], f"{tag} padded slots poked: grad {n}", label="tcl training: padded slots carry no gradient (scaled bar)")


# ---- 3. p = 0 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gen_k5_l1_h2", "hub_k10_l3_h4"])
def test_train_forward_at_p0_equals_inference(name):
    c, cfg, m = _train_case(name)
    a = (c["src"], c["dst"], c["times"])
    s, d = m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=cfg["K"])
    with torch.no_grad():
        es, ed = m.eval().compute_src_dst_node_temporal_embeddings(*a, num_neighbors=cfg["K"])
    e1 = close(s.detach().cpu().numpy(), es.cpu().numpy(), f"{name} train(p=0) src vs inference", "tcl training forward at p = 0 vs inference")
    e2 = close(d.detach().cpu().numpy(), ed.cpu().numpy(), f"{name} train(p=0) dst vs inference", "tcl training forward at p = 0 vs inference")
    print(f"{name}: max |train(p=0) - inference| = {max(e1, e2):.3e}")


# ---- 4. dropout ----------------------------------------------------------------------------------------------------------------------------------
# The seed of (bip_k20_l2_h2, 0.5) is not 0x123456c like its neighbours': with that seed ONE hidden unit of the oracle (layer 0, cross stage) has
# the pre-activation -2.7e-8, below what an fp32 product over 172 terms resolves, and the ReLU's gradient is discontinuous there.  The HIP
# path lands on the other side of the kink; opening that one gate in an fp64 run of the oracle reproduces the whole difference (time encoder
# weight gradient: 3.766e2 on 2.57e6, against a bar of 2.57e2; first elements +140.6, +60.8, +113.1, -29.9 against the observed +140.3,
# +60.7, +114.0, -29.3), while the oracle's own fp32 error is 1.2.  Such a case tests the kink, not the code.  Among the next candidate seeds
# 0x1234594 is the one whose smallest |pre-activation| in the fp64 oracle is largest (3.5e-7): chosen from the oracle alone.
DROPOUT_CASES = [("gen_k5_l1_h2", 0.1, 0x1234568), ("gen_k5_l1_h2", 0.5, 0x123456c), ("bip_k20_l2_h2", 0.1, 0x1234568), ("bip_k20_l2_h2", 0.5, 0x1234594)]


@pytest.mark.parametrize("name,p,seed", DROPOUT_CASES, ids=[f"{n}-{p}" for n, p, _ in DROPOUT_CASES])
def test_dropout_matches_oracle(name, p, seed):
    c, cfg, m = _train_case(name, p, seed)
    s, d = m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=cfg["K"])
    _fixture_loss(s, d).backward()
    got = _grads(m)
    ws, wd, _, ref = oracle_grads(c, OracleSampler(c["data"], cfg["strategy"], cfg["sampler_seed"]), p, seed)
    close(s.detach().cpu().numpy(), ws, f"{name} p={p} src vs oracle", "tcl training embeddings with dropout vs oracle")
    close(d.detach().cpu().numpy(), wd, f"{name} p={p} dst vs oracle", "tcl training embeddings with dropout vs oracle")
    for n, r in ref.items():
        close_scaled(got[n], r, f"{name} p={p} grad {n}", label="tcl training gradients with dropout vs oracle autograd (scaled bar)")


def test_dropout_seeds():
    c, cfg, m = _train_case("gen_k5_l1_h2", 0.1, 11)
    a = (c["src"], c["dst"], c["times"])
    s1, d1 = m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=cfg["K"])
    s2, d2 = m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=cfg["K"])
    m._fixed_dropout_seed = 12
    s3, d3 = m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=cfg["K"])
    assert torch.equal(s1, s2) and torch.equal(d1, d2)
    assert float((s1 - s3).abs().max()) > 1e-3 and float((d1 - d3).abs().max()) > 1e-3
    m._fixed_dropout_seed = None                                          # seeds from torch's generator
    torch.manual_seed(3)
    s4, _ = m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=cfg["K"])
    s5, _ = m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=cfg["K"])
    torch.manual_seed(3)
    s6, _ = m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=cfg["K"])
    assert not torch.equal(s4, s5) and torch.equal(s4, s6)


# ---- 5. two calls, one backward ---------------------------------------------------------------------------------------------------------------
def test_two_calls_one_backward():
    c, cfg, m = _train_case("bip_k20_l2_h2", 0.1, 21)
    K = cfg["K"]
    neg = lambda: m.compute_src_dst_node_temporal_embeddings(c["src"], c["neg_dst"], c["times"], num_neighbors=K)
    pos = lambda: m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=K)
    B = len(c["src"])
    parts = []
    for call, seeds in ((neg, (5, 6)), (pos, (7, 8))):
        m.zero_grad(set_to_none=True)
        _loss(*call(), seeds).backward()
        parts.append(_grads(m))
    m.zero_grad(set_to_none=True)
    ns, nd = neg()
    ps, pd = pos()                                                         # the first call's workspace must survive this one
    (_loss(ns, nd, (5, 6)) + _loss(ps, pd, (7, 8))).backward()
    both = _grads(m)
    assert B > 0 and any(np.abs(parts[0][n] - parts[1][n]).max() > 1e-3 for n in both)
    for n in both:
        close_scaled(both[n], parts[0][n] + parts[1][n], f"two calls grad {n}", label="tcl training: two calls, one backward (scaled bar)")


# ---- 6. guards ------------------------------------------------------------------------------------------------------------------------------------
def test_guards():
    name = "gen_k5_l1_h2"
    c, cfg, m = _train_case(name, 0.1, 31)
    K = cfg["K"]
    a = (c["src"], c["dst"], c["times"])
    s, d = m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=K)
    with torch.no_grad():
        m.output_layer.bias.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (s.sum() + d.sum()).backward()
    with torch.no_grad():
        m.output_layer.bias.sub_(1.0)
    with pytest.raises(NotImplementedError):
        m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=K, taps=2)
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.compute_step_embeddings(c["src"], c["dst"], c["neg_dst"], c["times"], num_neighbors=K)
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.eval().compute_src_dst_node_temporal_embeddings(*a, num_neighbors=K)
    m.train()
    with pytest.raises(AssertionError, match="num_depths"):
        m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=K + 1)
    # an empty batch takes part in autograd without a launch
    m.zero_grad(set_to_none=True)
    es, ed = m.compute_src_dst_node_temporal_embeddings(c["src"][:0], c["dst"][:0], c["times"][:0], num_neighbors=K)
    assert es.shape == ed.shape == (0, 172) and es.requires_grad
    (es.sum() + ed.sum()).backward()
    assert all(p.grad is None or not bool(p.grad.any()) for p in m.parameters())
    # a training step leaves the inference path as it was
    s, d = m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=K)
    _fixture_loss(s, d).backward()
    assert all(p.grad is not None for p in m.parameters())
    g = gc.load_golden(f"tcl_{name}")
    with torch.no_grad():
        for training in (True, False):
            s, d = m.train(training).compute_src_dst_node_temporal_embeddings(*a, num_neighbors=K)
            close(s.cpu().numpy(), g["src_emb"], f"{name} inference after a training step: src", "tcl embeddings vs reference")
            close(d.cpu().numpy(), g["dst_emb"], f"{name} inference after a training step: dst", "tcl embeddings vs reference")


# ---- 7. Adam ----------------------------------------------------------------------------------------------------------------------------------------
def test_adam_steps_reduce_the_loss():
    from dyglib_amd import MergeLayer
    torch.manual_seed(0)
    K, B = 5, 50
    data, nf, ef = syn.make_bipartite_graph(60, 15, 1500, seed=8)
    m = make_model(nf, ef, data, syn.make_tcl_params(9, K, num_layers=1), K, 1, 2).train()
    assert m.dropout == 0.1
    merge = MergeLayer(172, 172, 172, 1).to(DEV).train()
    opt = torch.optim.Adam(list(m.parameters()) + list(merge.parameters()), lr=1e-3)
    rs = np.random.RandomState(0)
    items = np.unique(data.dst_node_ids)
    losses = []
    for i in range(30):
        sl = slice(i * B, (i + 1) * B)
        src, dst, t = data.src_node_ids[sl], data.dst_node_ids[sl], data.node_interact_times[sl]
        neg = rs.choice(items, size=B)
        opt.zero_grad()
        ns, nd = m.compute_src_dst_node_temporal_embeddings(src, neg, t, num_neighbors=K)
        ps, pd = m.compute_src_dst_node_temporal_embeddings(src, dst, t, num_neighbors=K)
        pos, ng = merge(ps, pd).squeeze(-1).sigmoid(), merge(ns, nd).squeeze(-1).sigmoid()
        loss = torch.nn.functional.binary_cross_entropy(torch.cat([pos, ng]), torch.cat([torch.ones_like(pos), torch.zeros_like(ng)]))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert np.isfinite(losses).all()
    print(f"tcl adam: first 5 {np.mean(losses[:5]):.4f}, last 5 {np.mean(losses[-5:]):.4f}")
    assert np.mean(losses[-5:]) < np.mean(losses[:5]), losses


# ---- 8. the example ---------------------------------------------------------------------------------------------------------------------------------
def test_example_trains_tcl():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_link_prediction_synthetic.py"), "--model", "TCL", "--epochs", "1",
                        "--users", "60", "--items", "15", "--edges", "1500", "--batch", "50", "--num-neighbors", "5"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    hist = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(hist) == 1 and np.isfinite([hist[0]["train_loss"], hist[0]["val_ap"], hist[0]["val_auc"]]).all(), r.stdout
