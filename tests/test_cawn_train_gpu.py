"""CAWN training on the HIP path (dygnn_cawn_train_forward / dygnn_cawn_backward, dyglib_amd/csrc/cawn_train.hip, through
_CawnTrainFunction after enable_training()) on an MI355X: against the reference's own autograd (tests/golden/grads_cawn_<case>.npz) at p = 0,
against the differentiable restatement (tests/cawn_train_oracle.py, pinned to the same fixtures by tests/test_cawn_grads_cpu.py) with dropout
and at shapes that have no fixture, plus the autograd plumbing (two calls before one backward, guards, empty batches, the opt-in switch).
Bars: tests/parity.py, plain 1e-4 on forward quantities, 1e-4 * max(1, max |ref|) on gradients (weight gradients are atomic sums: never
compared for equality).  Every test builds its own model: the cached ones of tests/test_cawn_gpu.py stay as they are (training off)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dyglib_amd import synthetic as syn
from oracle.dropout import Drop
from tests import cawn_cases as cc
from tests import cawn_edge_cases as ce
from tests import cawn_oracle as cwo
from tests import cawn_train_oracle as cto
from tests import golden_cases as gc
from tests.parity import close, close_scaled
from tests.test_cawn_grads_cpu import oracle_grads
from tests.test_gradients_golden import _check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REV_HH = ("walk_encoder.feature_encoder.bilstm_encoder.weight_hh_l0_reverse", "walk_encoder.position_encoder.bilstm_encoder.weight_hh_l0_reverse")


def _grads(model):
    return {n: (None if p.grad is None else p.grad.detach().cpu().numpy()) for n, p in model.named_parameters()}


def _fixture_loss(s, d):
    G1, G2 = gc.grad_loss_weights(s.shape[0])
    return (s * torch.from_numpy(G1).to(s.device)).sum() + (d * torch.from_numpy(G2).to(d.device)).sum()


def _loss(s, d, seeds, rows=None):
    B, F = s.shape
    w = [torch.from_numpy(np.random.RandomState(x).standard_normal((B, F)).astype(np.float32)).to(s.device) for x in seeds]
    if rows is not None:
        for x in w:
            x[rows:] = 0.0
    return (s * w[0]).sum() + (d * w[1]).sum()


def make_model(data, node_feat, edge_feat, params, Ft, P, W, heads, strategy="recent", scale=0.0, seed=1, p=0.0, drop_seed=None):
    """a fresh model in train mode with training enabled"""
    from dyglib_amd import CAWN, get_neighbor_sampler
    sampler = get_neighbor_sampler(data, strategy, time_scaling_factor=scale, seed=seed, device=DEV)
    m = CAWN(node_feat, edge_feat, sampler, Ft, P, walk_length=W, num_walk_heads=heads, dropout=p, device=DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    m = m.to(DEV).train()
    if drop_seed is not None:
        m._fixed_dropout_seed = drop_seed
    return m


def _train_case(name, p=0.0, seed=None, enable=True):
    c = cc.build_cawn_case(name)
    cfg = c["cawn_cfg"]
    m = make_model(c["data"], c["node_feat"], c["edge_feat"], c["cawn_params"], cc.TIME_FEAT_DIM, cfg["P"], cfg["W"], cfg["heads"], cfg["strategy"],
                   cfg["scale"], cfg["sampler_seed"], p, seed)
    m.set_neighbor_sampler(m.neighbor_sampler)
    return c, cfg, (m.enable_training() if enable else m)


def _case_sides(c):
    """the `recent` hops of a fixture batch as sides [src ; dst], from the host sampler"""
    cfg = c["cawn_cfg"]
    return ce.batch_sides(c["data"], cfg["W"], cfg["k"], c["src"].astype(np.int64), c["dst"].astype(np.int64), c["times"])[0]


def hip_sides_run(m, sides, k, loss_seeds, p=0.0, seed=0, rows=None):
    """_CawnTrainFunction on explicit sides [src ; dst] -> (src_emb, dst_emb, grads) as numpy"""
    from dyglib_amd.cawn import _CawnTrainFunction
    roots, times, hops = sides
    B = len(roots) // 2
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    on_dev = (dev(roots), dev(times), [tuple(dev(x) for x in h) for h in hops])
    m.zero_grad(set_to_none=True)
    s, d = _CawnTrainFunction.apply(m, on_dev, B, k, float(p), int(seed), *m.parameters())
    _loss(s, d, loss_seeds, rows).backward()
    return s.detach().cpu().numpy(), d.detach().cpu().numpy(), _grads(m)


def oracle_sides_run(params, node_feat, edge_feat, sides, heads, loss_seeds, p=0.0, seed=0, rows=None):
    """the restatement's autograd on the same sides and the same loss; the reverse hidden weights, which it never reads, get zeros"""
    roots, times, hops = sides
    B = len(roots) // 2
    P = {n: torch.from_numpy(v.copy()).requires_grad_(True) for n, v in params.items()}
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    half = lambda sl: [(t(n[sl]), t(e[sl]), t(ts[sl])) for n, e, ts in hops]
    drop = Drop(p, seed) if p > 0 else None
    s, d = cto.forward(P, t(np.asarray(node_feat, np.float32)), t(np.asarray(edge_feat, np.float32)), t(roots[:B]), t(roots[B:]), t(times[:B]),
                       half(slice(0, B)), half(slice(B, 2 * B)), heads, drop)
    _loss(s, d, loss_seeds, rows).backward()
    grads = {n: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape), np.float32)) for n, v in P.items()}
    assert all(P[n].grad is not None or n in REV_HH for n in P)
    return s.detach().numpy(), d.detach().numpy(), grads


def compare(tag, got, want, label):
    close(got[0], want[0], f"{tag} src vs oracle", f"cawn training embeddings vs oracle ({label})")
    close(got[1], want[1], f"{tag} dst vs oracle", f"cawn training embeddings vs oracle ({label})")
    assert set(got[2]) == set(want[2]) and len(got[2]) == 38
    for n, r in want[2].items():
        assert got[2][n] is not None, n
        close_scaled(got[2][n], r, f"{tag} grad {n}", label=f"cawn training gradients vs oracle autograd ({label}, scaled bar)")
    for n in REV_HH:
        assert not got[2][n].any(), n


# ---- 1. p = 0: the inference forward and the reference's embeddings ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.CASES))
def test_train_forward_at_p0_equals_inference_and_reference(name):
    c, cfg, m = _train_case(name)
    g = gc.load_golden(f"cawn_{name}")
    a = (c["src"], c["dst"], c["times"])
    s, d = m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=cfg["k"])
    assert s.requires_grad and d.requires_grad
    m.set_neighbor_sampler(m.neighbor_sampler)                            # a random sampler draws the same hops again
    with torch.no_grad():
        es, ed = m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=cfg["k"])
    e1 = close(s.detach().cpu().numpy(), es.cpu().numpy(), f"{name} train(p=0) src vs inference", "cawn training forward at p = 0 vs inference")
    e2 = close(d.detach().cpu().numpy(), ed.cpu().numpy(), f"{name} train(p=0) dst vs inference", "cawn training forward at p = 0 vs inference")
    close(s.detach().cpu().numpy(), g["src_emb"], f"{name} train(p=0) src vs reference", "cawn training embeddings vs reference")
    close(d.detach().cpu().numpy(), g["dst_emb"], f"{name} train(p=0) dst vs reference", "cawn training embeddings vs reference")
    print(f"{name}: max |train(p=0) - inference| = {max(e1, e2):.3e}")


# ---- 2. the reference's own gradients --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.CASES))
def test_gradients_match_reference_autograd(name):
    """also the padding of gen_w1_k5 (first edges of the stream: empty histories on one and on both sides) and the partial walks and shared
    nodes of hub_w2_k4, both through the reference's own numbers"""
    c, cfg, m = _train_case(name)
    g = gc.load_golden(f"grads_cawn_{name}")
    s, d = m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=cfg["k"])
    close(s.detach().cpu().numpy(), g["src_emb"], f"{name} train src_emb", "cawn training embeddings vs reference")
    close(d.detach().cpu().numpy(), g["dst_emb"], f"{name} train dst_emb", "cawn training embeddings vs reference")
    _fixture_loss(s, d).backward()
    grads = _grads(m)
    assert all(v is not None for v in grads.values()) and set(grads) == set(c["cawn_params"]) and len(grads) == 38
    assert np.abs(grads["time_encoder.w.weight"]).max() > 0 and np.abs(grads["time_encoder.w.bias"]).max() > 0      # CAWN's time encoder trains
    for n in REV_HH:
        assert grads[n].shape == c["cawn_params"][n].shape and not grads[n].any(), n      # a zero tensor, not None, as in the reference
    for enc in ("feature_encoder", "position_encoder"):
        for suffix in ("", "_reverse"):
            p = f"walk_encoder.{enc}.bilstm_encoder."
            assert np.array_equal(grads[p + "bias_ih_l0" + suffix], grads[p + "bias_hh_l0" + suffix])               # one sum, written to both
    _check(f"cawn hip {name}", grads, g)
    if cfg["strategy"] != "recent":                       # the RandomState was consumed as by the reference's call
        with torch.no_grad():
            sn, nd = m.compute_src_dst_node_temporal_embeddings(c["src"], c["neg_dst"], c["times"], num_neighbors=cfg["k"])
        close(sn.cpu().numpy(), g["src_neg_emb"], f"{name} src_neg_emb after the training call", "cawn training embeddings vs reference")
        close(nd.cpu().numpy(), g["neg_dst_emb"], f"{name} neg_dst_emb after the training call", "cawn training embeddings vs reference")


# ---- 3. dropout ----------------------------------------------------------------------------------------------------------------------------------
DROPOUT_CASES = [("gen_w1_k5", 0.1, 0x1234568), ("gen_w1_k5", 0.5, 0x123456c), ("hub_w2_k4", 0.1, 0x1234568), ("hub_w2_k4", 0.5, 0x123456c)]


@pytest.mark.parametrize("name,p,seed", DROPOUT_CASES, ids=[f"{n}-{p}" for n, p, _ in DROPOUT_CASES])
def test_dropout_matches_oracle(name, p, seed):
    c, cfg, m = _train_case(name, p, seed)
    s, d = m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=cfg["k"])
    _fixture_loss(s, d).backward()
    got = _grads(m)
    ws, wd, _, ref = oracle_grads(c, cwo.OracleSampler(c["data"], cfg["strategy"], cfg["sampler_seed"], cfg["scale"]), p, seed)
    close(s.detach().cpu().numpy(), ws, f"{name} p={p} src vs oracle", "cawn training embeddings with dropout vs oracle")
    close(d.detach().cpu().numpy(), wd, f"{name} p={p} dst vs oracle", "cawn training embeddings with dropout vs oracle")
    base = gc.load_golden(f"cawn_{name}")["src_emb"]
    assert np.abs(ws - base).max() > 1e-2                                 # the masks do something
    for n, r in ref.items():
        close_scaled(got[n], r, f"{name} p={p} grad {n}", label="cawn training gradients with dropout vs oracle autograd (scaled bar)")


def test_dropout_seeds():
    c, cfg, m = _train_case("hub_w2_k4", 0.1, 11)
    a = (c["src"], c["dst"], c["times"])
    call = lambda: m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=cfg["k"])
    s1, d1 = call()
    s2, d2 = call()
    m._fixed_dropout_seed = 12
    s3, d3 = call()
    assert torch.equal(s1, s2) and torch.equal(d1, d2)
    assert float((s1 - s3).detach().abs().max()) > 1e-3 and float((d1 - d3).detach().abs().max()) > 1e-3
    m._fixed_dropout_seed = None                                          # seeds from torch's generator
    torch.manual_seed(3)
    s4, s5 = call()[0], call()[0]
    torch.manual_seed(3)
    s6 = call()[0]
    assert not torch.equal(s4, s5) and torch.equal(s4, s6)


# ---- 4. two calls, one backward ---------------------------------------------------------------------------------------------------------------
def test_two_calls_one_backward():
    c, cfg, m = _train_case("hub_w2_k4", 0.1, 21)
    k = cfg["k"]
    neg = lambda: m.compute_src_dst_node_temporal_embeddings(c["src"], c["neg_dst"], c["times"], num_neighbors=k)
    pos = lambda: m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=k)
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
    assert any(np.abs(parts[0][n] - parts[1][n]).max() > 1e-3 for n in both)
    for n in both:
        close_scaled(both[n], parts[0][n] + parts[1][n], f"two calls grad {n}", label="cawn training: two calls, one backward (scaled bar)")


# ---- 5. padding and the position scatter, against the restatement -----------------------------------------------------------------------------
def _fresh(c, cfg, p=0.0):
    return make_model(c["data"], c["node_feat"], c["edge_feat"], c["cawn_params"], cc.TIME_FEAT_DIM, cfg["P"], cfg["W"], cfg["heads"], p=p).enable_training()


def test_partial_walks_and_shared_nodes_match_the_oracle_and_padded_slots_carry_no_gradient():
    """hub_w2_k4: partial walks [t, x, 0], one-sided pairs, the hub items at several hops of both trees of a pair (several tree positions per
    dPF row).  Then every padded slot of the call gets another edge id and another time (the ids stay 0: that is what makes a slot padded):
    neither the embeddings nor any gradient may move."""
    c = cc.build_cawn_case("hub_w2_k4")
    cfg = c["cawn_cfg"]
    sides = _case_sides(c)
    roots, times, hops = sides
    T2 = np.concatenate([roots[:, None]] + [h[0] for h in hops], axis=1)
    B = len(c["src"])
    shared = [len(np.intersect1d(T2[i][T2[i] != 0], T2[B + i][T2[B + i] != 0])) for i in range(B)]
    assert max(shared) >= 2 and ((hops[0][0] != 0) & (hops[1][0].reshape(2 * B, cfg["k"], cfg["k"]) == 0).any(-1)).any()
    m = _fresh(c, cfg)
    got = hip_sides_run(m, sides, cfg["k"], (1, 2))
    want = oracle_sides_run(c["cawn_params"], c["node_feat"], c["edge_feat"], sides, cfg["heads"], (1, 2))
    compare("hub_w2_k4 sides", got, want, "padding, shared nodes")
    rs = np.random.RandomState(5)
    poked = []
    for n, e, t in hops:
        pad = n == 0
        assert pad.any()
        poked.append((n, np.where(pad, rs.randint(1, c["edge_feat"].shape[0], e.shape), e), np.where(pad, rs.uniform(0, 1e6, t.shape), t).astype(np.float32)))
    again = hip_sides_run(m, (roots, times, poked), cfg["k"], (1, 2))
    close(again[0], got[0], "padded slots poked: src", "cawn training: padded slots do not reach the embeddings")
    close(again[1], got[1], "padded slots poked: dst", "cawn training: padded slots do not reach the embeddings")
    for n in got[2]:
        close_scaled(again[2][n], got[2][n], f"padded slots poked: grad {n}", label="cawn training: padded slots carry no gradient (scaled bar)")


def test_identical_trees_of_a_pair():
    """src == dst at the same time: both trees of the pair are identical, every unique id has positions in both, and both count rows are equal"""
    c = cc.build_cawn_case("hub_w2_k4")
    cfg = c["cawn_cfg"]
    src = c["src"][-3:].astype(np.int64)
    sides = ce.batch_sides(c["data"], cfg["W"], cfg["k"], src, src.copy(), c["times"][-3:])[0]
    assert all(np.array_equal(h[0][:3], h[0][3:]) for h in sides[2]) and (sides[2][0][0] != 0).any()
    m = _fresh(c, cfg)
    got = hip_sides_run(m, sides, cfg["k"], (3, 4))
    want = oracle_sides_run(c["cawn_params"], c["node_feat"], c["edge_feat"], sides, cfg["heads"], (3, 4))
    compare("src == dst", got, want, "identical trees")


# ---- 6. edge shapes, against the restatement ------------------------------------------------------------------------------------------------------
# tests/cawn_edge_cases.py SHAPES: M = 64 both ways (the largest the training path accepts), D = 72 with one head of 36 and H_p = 4,
# attention_dim 512 with head size 64 (the fc1 product's K = 2048), attention_dim 260 (five columns per lane in the LayerNorm rows)
@pytest.mark.parametrize("name", ["w2_k8", "w1_k64", "narrow_h1", "all256_h8", "P76_h5"])
def test_edge_shapes_match_oracle(name):
    c = ce.shape_case(name)
    r = c["cfg"]
    m = make_model(c["data"], c["node_feat"], c["edge_feat"], c["params"], r["Ft"], r["P"], r["W"], r["heads"]).enable_training()
    got = hip_sides_run(m, c["sides"], r["k"], (1, 2))
    want = oracle_sides_run(c["params"], c["node_feat"], c["edge_feat"], c["sides"], r["heads"], (1, 2))
    compare(name, got, want, "edge shapes")


def _small_case(W, k, P, heads, B):
    """shape_case's bipartite graph with a model of the default feature dims; the first pair has empty histories"""
    rs = np.random.RandomState(4)
    data, nf, ef = syn.make_bipartite_graph(60, 9, 6000, seed=3, duplicate_time_every=5, edge_feat_dim=172)
    nf = (0.5 * rs.standard_normal((nf.shape[0], 172))).astype(np.float32)
    nf[0] = 0.0
    idx = rs.randint(0, data.num_interactions, B)
    times = data.node_interact_times[idx].astype(np.float64)
    if B > 1:
        times[0] = data.node_interact_times.min() - 1.0              # both histories empty
    src, dst = data.src_node_ids[idx].astype(np.int64), data.dst_node_ids[idx].astype(np.int64)
    return dict(data=data, node_feat=nf, edge_feat=ef, src=src, dst=dst, times=times, params=syn.make_cawn_params(ce.PARAM_SEED, P, W, heads),
                sides=ce.batch_sides(data, W, k, src, dst, times)[0])


SMALL = [  # W, k, P, heads, B
    (1, 1, 172, 8, 3),       # M = 1: one walk, a softmax over one key
    (2, 3, 6, 4, 4),         # position_feat_dim 6: rows 8-byte aligned only, H_p = 3, D = 450 (2 mod 4): the general products, not the grouped one
    (2, 4, 24, 4, 1),        # B = 1; attention_dim 236, head size 59
    (1, 32, 172, 8, 2),      # the Wikipedia configuration: attention_dim 312, head size 39
]


@pytest.mark.parametrize("W,k,P,heads,B", SMALL, ids=[f"W{s[0]}-k{s[1]}-P{s[2]}-B{s[4]}" for s in SMALL])
def test_small_shapes_match_oracle(W, k, P, heads, B):
    c = _small_case(W, k, P, heads, B)
    m = make_model(c["data"], c["node_feat"], c["edge_feat"], c["params"], cc.TIME_FEAT_DIM, P, W, heads).enable_training()
    got = hip_sides_run(m, c["sides"], k, (1, 2))
    want = oracle_sides_run(c["params"], c["node_feat"], c["edge_feat"], c["sides"], heads, (1, 2))
    compare(f"W{W} k{k} P{P} B{B}", got, want, "small shapes")
    # and through the class, which samples the same `recent` hops on the device
    m.zero_grad(set_to_none=True)
    s, d = m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=k)
    close(s.detach().cpu().numpy(), want[0], f"W{W} k{k} P{P} B{B} class src", "cawn training embeddings vs oracle (small shapes)")


# ---- 7. guards ------------------------------------------------------------------------------------------------------------------------------------
def test_guards_and_the_switch():
    name = "gen_w1_k5"
    c, cfg, m = _train_case(name, 0.1, 31, enable=False)
    k = cfg["k"]
    a = (c["src"], c["dst"], c["times"])
    with pytest.raises(NotImplementedError, match="inference-only"):       # training off: as before this path existed
        m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=k)
    assert m.enable_training() is m
    s, d = m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=k)
    with torch.no_grad():
        m.walk_encoder.projection_layers[1].bias.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (s.sum() + d.sum()).backward()
    with torch.no_grad():
        m.walk_encoder.projection_layers[1].bias.sub_(1.0)
    with pytest.raises(NotImplementedError, match="taps"):
        m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=k, taps=2)
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.compute_step_embeddings(c["src"], c["dst"], c["neg_dst"], c["times"], num_neighbors=k)
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.eval().compute_src_dst_node_temporal_embeddings(*a, num_neighbors=k)
    m.train()
    with pytest.raises(NotImplementedError, match=r"65 walks \(num_neighbors 65 \*\* walk_length 1\) > 64 not supported by the training path"):
        m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=65)
    with torch.no_grad():                                                  # the inference forward still takes 65 walks
        m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=65)
    # an empty batch takes part in autograd without a launch
    m.zero_grad(set_to_none=True)
    es, ed = m.compute_src_dst_node_temporal_embeddings(c["src"][:0], c["dst"][:0], c["times"][:0], num_neighbors=k)
    assert es.shape == ed.shape == (0, 172) and es.requires_grad
    (es.sum() + ed.sum()).backward()
    assert all(p.grad is None or not bool(p.grad.any()) for p in m.parameters())
    # a training step leaves the inference path as it was, and switching off restores the refusal
    s, d = m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=k)
    _fixture_loss(s, d).backward()
    assert all(p.grad is not None for p in m.parameters())
    g = gc.load_golden(f"cawn_{name}")
    with torch.no_grad():
        for training in (True, False):
            s, d = m.train(training).compute_src_dst_node_temporal_embeddings(*a, num_neighbors=k)
            close(s.cpu().numpy(), g["src_emb"], f"{name} inference after a training step: src", "cawn embeddings vs reference")
            close(d.cpu().numpy(), g["dst_emb"], f"{name} inference after a training step: dst", "cawn embeddings vs reference")
    m.train().enable_training(False)
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.compute_src_dst_node_temporal_embeddings(*a, num_neighbors=k)


# ---- 8. Adam ----------------------------------------------------------------------------------------------------------------------------------------
def test_adam_steps_reduce_the_loss():
    from dyglib_amd import MergeLayer
    torch.manual_seed(0)
    k, B = 4, 50
    data, nf, ef = syn.make_bipartite_graph(60, 15, 1500, seed=8)
    m = make_model(data, nf, ef, syn.make_cawn_params(9, 24, 1, 4), cc.TIME_FEAT_DIM, 24, 1, 4, p=0.1).enable_training()
    merge = MergeLayer(172, 172, 172, 1).to(DEV).train()
    opt = torch.optim.Adam(list(m.parameters()) + list(merge.parameters()), lr=1e-3)
    rs = np.random.RandomState(0)
    items = np.unique(data.dst_node_ids)
    losses = []
    for i in range(1, 25):
        sl = slice(i * B, (i + 1) * B)
        src, dst, t = data.src_node_ids[sl], data.dst_node_ids[sl], data.node_interact_times[sl]
        neg = rs.choice(items, size=B)
        opt.zero_grad()
        ns, nd = m.compute_src_dst_node_temporal_embeddings(src, neg, t, num_neighbors=k)
        ps, pd = m.compute_src_dst_node_temporal_embeddings(src, dst, t, num_neighbors=k)
        pos, ng = merge(ps, pd).squeeze(-1).sigmoid(), merge(ns, nd).squeeze(-1).sigmoid()
        loss = torch.nn.functional.binary_cross_entropy(torch.cat([pos, ng]), torch.cat([torch.ones_like(pos), torch.zeros_like(ng)]))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert np.isfinite(losses).all()
    print(f"cawn adam: first 5 {np.mean(losses[:5]):.4f}, last 5 {np.mean(losses[-5:]):.4f}")
    assert np.mean(losses[-5:]) < np.mean(losses[:5]), losses


# ---- 9. the example ---------------------------------------------------------------------------------------------------------------------------------
def test_example_trains_cawn():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_link_prediction_synthetic.py"), "--model", "CAWN", "--epochs", "1",
                        "--users", "60", "--items", "15", "--edges", "1500", "--batch", "50", "--num-neighbors", "5"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    hist = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(hist) == 1 and np.isfinite([hist[0]["train_loss"], hist[0]["val_ap"], hist[0]["val_auc"]]).all(), r.stdout
