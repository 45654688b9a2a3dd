"""GraphMixer training on the HIP path (dygnn_graphmixer_train_forward / dygnn_graphmixer_backward, dyglib_amd/csrc/graphmixer_train.hip,
through _GraphMixerTrainFunction) on an MI355X: against the reference's own autograd (tests/golden/grads_graphmixer_<case>.npz) at p = 0,
against the differentiable restatement (tests/graphmixer_train_oracle.py, pinned to the same fixtures by tests/test_graphmixer_grads_cpu.py)
at shapes that have no fixture and with dropout, plus the autograd plumbing (two calls before one backward, independence of the roots,
guards) and the example.  Bars: tests/parity.py, plain 1e-4 on forward quantities, 1e-4 * max(1, max |ref|) on gradients (the four big
weight gradients are atomic sums: never compared for equality).  The observed maxima are printed at the end of the run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dyglib_amd import _capi, synthetic as syn
from oracle import dygformer_oracle as orc
from tests import golden_cases as gc
from tests import graphmixer_train_oracle as gto
from tests.parity import close, close_scaled
from tests.test_gradients_golden import _check
from tests.test_graphmixer_gpu import DEV, case_model, make_model
from tests.test_graphmixer_grads_cpu import GRAD_CASES, case, oracle_grads, trainable

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FROZEN = ("time_encoder.w.weight", "time_encoder.w.bias")


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
    return c, cfg, m


def _check_frozen_and_live(grads, tag):
    for n, g in grads.items():
        if n in FROZEN:
            assert g is None, (tag, n)                                   # as in the reference: .grad stays None
        else:
            assert g is not None and np.isfinite(g).all() and np.abs(g).max() > 0, (tag, n)


# ---- 1. the reference's own gradients --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAD_CASES)
def test_gradients_match_reference_autograd(name):
    c, cfg, m = _train_case(name)
    g = gc.load_golden(f"grads_graphmixer_{name}")
    kw = dict(num_neighbors=cfg["K"], time_gap=cfg["G"])
    s, d = m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], **kw)
    assert s.requires_grad and d.requires_grad
    close(s.detach().cpu().numpy(), g["src_emb"], f"{name} train src_emb", "graphmixer training embeddings vs reference")
    close(d.detach().cpu().numpy(), g["dst_emb"], f"{name} train dst_emb", "graphmixer training embeddings vs reference")
    _fixture_loss(s, d).backward()
    grads = _grads(m)
    assert set(grads) == set(c["gm_params"])
    _check_frozen_and_live(grads, name)
    _check(f"graphmixer hip {name}", {k: v for k, v in grads.items() if k not in FROZEN}, g)
    with torch.no_grad():
        es, ed = m.eval().compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], **kw)
    close(s.detach().cpu().numpy(), es.cpu().numpy(), f"{name} train(p=0) src vs inference", "graphmixer training forward at p = 0 vs inference")
    close(d.detach().cpu().numpy(), ed.cpu().numpy(), f"{name} train(p=0) dst vs inference", "graphmixer training forward at p = 0 vs inference")


# ---- 2. shapes without a fixture, against the restatement's autograd -----------------------------------------------------------------------------
_SETUPS = {}


def _setup(K, L, n, Fn, Cc, Ft):
    """a bipartite graph with non-zero node features (row 0 included), seeded parameters and n roots: interactions' endpoints at their own
    times (histories of every length); root 0 precedes every interaction (all K slots padded).  Built once per shape, left unchanged."""
    key = (K, L, n, Fn, Cc, Ft)
    if key not in _SETUPS:
        seed = 7
        data, nf, ef = syn.make_bipartite_graph(60, 9, 6000, seed=seed, duplicate_time_every=5)
        rs = np.random.RandomState(seed + 1)
        nf = (0.5 * rs.standard_normal((nf.shape[0], Fn))).astype(np.float32)
        ef = np.ascontiguousarray(ef[:, :Cc])
        params = syn.make_graphmixer_params(seed + 2, K, num_layers=L, node_feat_dim=Fn, edge_feat_dim=Cc, time_feat_dim=Ft)
        rs = np.random.RandomState(100 + n)
        idx = rs.randint(0, data.num_interactions, n)
        nodes = np.where(rs.randint(0, 2, n) == 0, data.src_node_ids[idx], data.dst_node_ids[idx]).astype(np.int64)
        times = data.node_interact_times[idx].astype(np.float64)
        times[0] = data.node_interact_times.min() - 1.0
        adj = orc.OracleAdjacency(data.src_node_ids, data.dst_node_ids, data.edge_ids, data.node_interact_times)
        _SETUPS[key] = dict(data=data, node_feat=nf, edge_feat=ef, params=params, nodes=nodes, times=times, adj=adj, K=K, L=L, Ft=Ft, G=50)
    return _SETUPS[key]


def _model(c, p=0.0, seed=None):
    m = make_model(c["node_feat"], c["edge_feat"], c["data"], c["params"], c["K"], c["L"], c["Ft"]).train()
    m.dropout = p
    if seed is not None:
        m._fixed_dropout_seed = seed
    return m


def _weights(shape, seed, dev="cpu"):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(tuple(shape)).astype(np.float32)).to(dev)


def _oracle(c, loss_seed, p=0.0, seed=0, nodes=None, times=None, rows=None):
    """(embeddings, {name: grad}) of the restatement; the loss is sum(emb * W(loss_seed)), over the first `rows` rows only if given"""
    nodes = c["nodes"] if nodes is None else nodes
    times = c["times"] if times is None else times
    P = trainable(c["params"])
    emb = gto.graphmixer_train_forward(P, c["node_feat"], c["edge_feat"], c["adj"], nodes, times, c["K"], c["G"], c["L"], p, seed)
    w = _weights(emb.shape, loss_seed)
    if rows is not None:
        w[rows:] = 0.0
    (emb * w).sum().backward()
    return emb.detach().numpy(), {k: (None if v.grad is None else v.grad.numpy()) for k, v in P.items()}


def _against_oracle(c, tag, p=0.0, seed=None):
    m = _model(c, p, seed)
    emb = m.compute_node_temporal_embeddings(c["nodes"], c["times"], num_neighbors=c["K"], time_gap=c["G"])
    (emb * _weights(emb.shape, 1, DEV)).sum().backward()
    got = _grads(m)
    want_emb, want = _oracle(c, 1, p, seed or 0)
    close(emb.detach().cpu().numpy(), want_emb, tag + " embeddings vs oracle", "graphmixer training embeddings vs oracle")
    assert set(got) == set(want)
    for k, ref in want.items():
        if k in FROZEN:
            assert got[k] is None and ref is None, k
        else:
            close_scaled(got[k], ref, f"{tag} grad {k}", label="graphmixer training gradients vs oracle autograd (scaled bar)")
    return m, emb


SHAPES = [  # K, blocks, n, Fn, C, Ft
    (2, 1, 1, 16, 16, 16),            # Kh = 1, one root (all padding), H = 64: a single hidden chunk
    (4, 3, 45, 64, 32, 16),           # Fn != C; n is a multiple of no tile; H = 128
    (32, 1, 21, 172, 172, 100),       # K at its maximum; H = 688
    (30, 2, 67, 172, 172, 100),       # R = 2010 is not a multiple of 64
    (10, _capi.DYGNN_MAX_LAYERS, 21, 172, 172, 100),
]


@pytest.mark.parametrize("shape", SHAPES, ids=["K%d-L%d-n%d-Fn%d-C%d-Ft%d" % s for s in SHAPES])
def test_gradients_match_oracle_autograd(shape):
    c = _setup(*shape)
    assert not orc.get_historical_neighbors_recent(c["adj"], c["nodes"][:1], c["times"][:1], c["K"])[0].any()      # the all-padding root is there
    _against_oracle(c, "graphmixer train K%d L%d n%d Fn%d C%d" % shape[:5])


# ---- 3. dropout ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_matches_oracle_on_a_fixture_case(p):
    name, seed = "gen_k10_g7", 0x1234568
    c, cfg, m = _train_case(name, p, seed)
    s, d = m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=cfg["K"], time_gap=cfg["G"])
    _fixture_loss(s, d).backward()
    got = _grads(m)
    ws, wd, _, ref = oracle_grads(case(name), p, seed)
    close(s.detach().cpu().numpy(), ws, f"{name} p={p} src vs oracle", "graphmixer training embeddings with dropout vs oracle")
    close(d.detach().cpu().numpy(), wd, f"{name} p={p} dst vs oracle", "graphmixer training embeddings with dropout vs oracle")
    for n, r in ref.items():
        if n in FROZEN:
            assert got[n] is None and r is None
        else:
            close_scaled(got[n], r, f"{name} p={p} grad {n}", label="graphmixer training gradients with dropout vs oracle autograd (scaled bar)")


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_matches_oracle_off_fixture(p):
    _against_oracle(_setup(30, 2, 67, 172, 172, 100), f"graphmixer train K30 L2 n67 p={p}", p, 0x1234568)


def test_dropout_seeds():
    c, cfg, m = _train_case("gen_k10_g7", 0.1, 11)
    a, kw = (c["src"], c["dst"], c["times"]), dict(num_neighbors=cfg["K"], time_gap=cfg["G"])
    s1, d1 = m.compute_src_dst_node_temporal_embeddings(*a, **kw)
    s2, d2 = m.compute_src_dst_node_temporal_embeddings(*a, **kw)
    m._fixed_dropout_seed = 12
    s3, d3 = m.compute_src_dst_node_temporal_embeddings(*a, **kw)
    assert torch.equal(s1, s2) and torch.equal(d1, d2)
    assert float((s1 - s3).detach().abs().max()) > 1e-3 and float((d1 - d3).detach().abs().max()) > 1e-3
    m._fixed_dropout_seed = None                                          # seeds from torch's generator
    torch.manual_seed(3)
    s4, _ = m.compute_src_dst_node_temporal_embeddings(*a, **kw)
    s5, _ = m.compute_src_dst_node_temporal_embeddings(*a, **kw)
    torch.manual_seed(3)
    s6, _ = m.compute_src_dst_node_temporal_embeddings(*a, **kw)
    assert not torch.equal(s4, s5) and torch.equal(s4, s6)


# ---- 4. two calls, one backward ---------------------------------------------------------------------------------------------------------------
def test_two_calls_one_backward():
    c, cfg, m = _train_case("bip_k30_g50", 0.1, 21)
    kw = dict(num_neighbors=cfg["K"], time_gap=cfg["G"])
    neg = lambda: m.compute_src_dst_node_temporal_embeddings(c["src"], c["neg_dst"], c["times"], **kw)
    pos = lambda: m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], **kw)
    loss = lambda s, d, seeds: (s * _weights(s.shape, seeds[0], DEV)).sum() + (d * _weights(d.shape, seeds[1], DEV)).sum()
    parts = []
    for call, seeds in ((neg, (5, 6)), (pos, (7, 8))):
        m.zero_grad(set_to_none=True)
        loss(*call(), seeds).backward()
        parts.append(_grads(m))
    m.zero_grad(set_to_none=True)
    ns, nd = neg()
    ps, pd = pos()                                                         # the first call's workspace must survive this one
    (loss(ns, nd, (5, 6)) + loss(ps, pd, (7, 8))).backward()
    both = _grads(m)
    live = [n for n in both if n not in FROZEN]
    assert len(c["src"]) > 0 and any(np.abs(parts[0][n] - parts[1][n]).max() > 1e-3 for n in live)
    for n in live:
        close_scaled(both[n], parts[0][n] + parts[1][n], f"two calls grad {n}", label="graphmixer training: two calls, one backward (scaled bar)")
    assert all(both[n] is None for n in FROZEN)


# ---- 5. a root's row and its gradients do not depend on the other roots of the call ----------------------------------------------------------------
@pytest.mark.parametrize("p,row", [(0.0, 13), (0.1, 0)], ids=["p0-row13", "p0.1-first"])
def test_gradients_of_one_root_do_not_depend_on_the_call(p, row):
    """the dropout masks are indexed by the root's place in the call, so with dropout the root stands first in both calls"""
    c = _setup(30, 2, 67, 172, 172, 100)
    nodes, times = c["nodes"].copy(), c["times"].copy()
    if row == 0:                                                           # a root with a history in front (root 0 of the setup has none)
        nodes[[0, 13]], times[[0, 13]] = nodes[[13, 0]], times[[13, 0]]
    m = _model(c, p, 77)
    kw = dict(num_neighbors=c["K"], time_gap=c["G"])
    w = _weights((1, 172), 9, DEV)
    runs = []
    for sel in (slice(None), slice(row, row + 1)):
        m.zero_grad(set_to_none=True)
        emb = m.compute_node_temporal_embeddings(nodes[sel], times[sel], **kw)
        r = row if emb.shape[0] > 1 else 0
        (emb[r:r + 1] * w).sum().backward()
        runs.append((emb[r].detach().cpu().numpy(), _grads(m)))
    close(runs[0][0], runs[1][0], f"one root of 67, p={p}: embedding", "graphmixer training: one root alone vs in a call")
    assert any(np.abs(runs[1][1][n]).max() > 0 for n in runs[1][1] if n not in FROZEN)
    for n, g in runs[1][1].items():
        if n not in FROZEN:
            close_scaled(runs[0][1][n], g, f"one root of 67, p={p}: grad {n}", label="graphmixer training: one root alone vs in a call (scaled bar)")


# ---- 6. guards ------------------------------------------------------------------------------------------------------------------------------------
def test_guards():
    from dyglib_amd import get_neighbor_sampler
    name = "gen_k10_g7"
    c, cfg, m = _train_case(name, 0.1, 31)
    a, kw = (c["src"], c["dst"], c["times"]), dict(num_neighbors=cfg["K"], time_gap=cfg["G"])
    s, d = m.compute_src_dst_node_temporal_embeddings(*a, **kw)
    with torch.no_grad():
        m.output_layer.bias.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (s.sum() + d.sum()).backward()
    with torch.no_grad():
        m.output_layer.bias.sub_(1.0)
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.compute_node_temporal_embeddings(c["src"], c["times"], taps=2, **kw)
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.compute_step_embeddings(c["src"], c["dst"], c["neg_dst"], c["times"], **kw)
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.eval().compute_src_dst_node_temporal_embeddings(*a, **kw)
    m.train()
    with pytest.raises(AssertionError, match="must equal num_tokens"):
        m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=cfg["K"] + 1, time_gap=cfg["G"])
    recent = m.neighbor_sampler
    m.set_neighbor_sampler(get_neighbor_sampler(c["data"], "uniform", seed=2, device=DEV))
    with pytest.raises(NotImplementedError, match="recent"):
        m.compute_src_dst_node_temporal_embeddings(*a, **kw)
    m.set_neighbor_sampler(recent)
    cpu = case_model(name)[2].to("cpu").train()
    with pytest.raises(_capi.DygnnError, match="no CPU fallback"):
        cpu.compute_src_dst_node_temporal_embeddings(*a, **kw)
    # an empty batch takes part in autograd without a launch
    m.zero_grad(set_to_none=True)
    es, ed = m.compute_src_dst_node_temporal_embeddings(c["src"][:0], c["dst"][:0], c["times"][:0], **kw)
    assert es.shape == ed.shape == (0, 172) and es.requires_grad
    (es.sum() + ed.sum()).backward()
    assert all(p.grad is None or not bool(p.grad.any()) for p in m.parameters())
    # compute_node_temporal_embeddings is differentiable too and agrees with the rows of the pair call (same place in the call: same masks)
    m.zero_grad(set_to_none=True)
    s, d = m.compute_src_dst_node_temporal_embeddings(*a, **kw)
    e = m.compute_node_temporal_embeddings(np.concatenate([c["src"], c["dst"]]), np.concatenate([c["times"], c["times"]]), **kw)
    assert e.requires_grad and torch.equal(e[:len(c["src"])], s) and torch.equal(e[len(c["src"]):], d)
    e.sum().backward()
    _check_frozen_and_live(_grads(m), "compute_node_temporal_embeddings")
    # a training step leaves the inference path as it was: train mode under no_grad is still the fixture forward
    g = gc.load_golden(f"graphmixer_{name}")
    with torch.no_grad():
        for training in (True, False):
            s, d = m.train(training).compute_src_dst_node_temporal_embeddings(*a, **kw)
            close(s.cpu().numpy(), g["src_emb"], f"{name} inference after a training step: src", "graphmixer embeddings vs reference")
            close(d.cpu().numpy(), g["dst_emb"], f"{name} inference after a training step: dst", "graphmixer embeddings vs reference")


# ---- 7. the example ---------------------------------------------------------------------------------------------------------------------------------
def test_example_trains_graphmixer():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_link_prediction_synthetic.py"), "--model", "GraphMixer", "--epochs", "1",
                        "--users", "60", "--items", "15", "--edges", "1500", "--batch", "50", "--num-neighbors", "5"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    hist = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(hist) == 1 and np.isfinite([hist[0]["train_loss"], hist[0]["val_ap"], hist[0]["val_auc"]]).all(), r.stdout
    print(f"graphmixer example: train loss {hist[0]['train_loss']:.4f}, val AP {hist[0]['val_ap']:.4f}, val AUC {hist[0]['val_auc']:.4f}")
    # above chance: as many negatives as positives.  Observed on an MI355X: train loss 0.6934, val AP 0.5262, val AUC 0.4992 (21 Adam steps at
    # lr 1e-4 from a fresh initialisation barely move the model; seeds are fixed, so the figure repeats up to the atomics' rounding)
    assert hist[0]["val_ap"] > 0.5, hist[0]
