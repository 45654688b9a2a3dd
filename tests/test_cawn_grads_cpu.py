"""The differentiable CAWN restatement (tests/cawn_train_oracle.py) without a GPU: at p = 0 against the reference's own autograd
(tests/golden/grads_cawn_<case>.npz, written by tools/make_golden_cawn_grads.py), two properties of those fixtures the HIP backward relies
on, and a self-check of the dropout sites."""
import numpy as np
import pytest
import torch

from tests import cawn_cases as cc
from tests import cawn_oracle as cwo
from tests import cawn_train_oracle as cto
from tests import golden_cases as gc
from tests import parity
from tests.test_cawn_cpu import oracle_call
from tests.test_gradients_golden import _check


def oracle_grads(c, smp, dropout_p=0.0, seed=0, src=None, dst=None, times=None):
    """(src_emb, dst_emb, loss, {name: grad}) of the fixture loss on the restatement"""
    cfg = c["cawn_cfg"]
    src, dst, times = (c["src"] if src is None else src), (c["dst"] if dst is None else dst), (c["times"] if times is None else times)
    P = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in c["cawn_params"].items()}
    a = smp.multi_hop(cfg["W"], src, times, cfg["k"])              # all hops of the sources, then of the destinations
    b = smp.multi_hop(cfg["W"], dst, times, cfg["k"])
    s, d = cto.cawn_train_forward(P, c["node_feat"], c["edge_feat"], src, dst, times, a, b, cfg["heads"], dropout_p, seed)
    G1, G2 = gc.grad_loss_weights(len(src))
    loss = (s * torch.from_numpy(G1)).sum() + (d * torch.from_numpy(G2)).sum()
    loss.backward()
    # the restatement's reverse direction is one cell from the zero state: it never reads weight_hh_l0_reverse, whose gradient is exactly zero
    zero_ok = lambda k: k.endswith("weight_hh_l0_reverse")
    return s.detach().numpy(), d.detach().numpy(), float(loss.detach()), {
        k: (p.grad.numpy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32) if zero_ok(k) else None) for k, p in P.items()}


@pytest.mark.parametrize("name", list(cc.CASES))
def test_oracle_autograd_matches_reference_gradients(name):
    c = cc.build_cawn_case(name)
    cfg = c["cawn_cfg"]
    g = gc.load_golden(f"grads_cawn_{name}")
    smp = cwo.OracleSampler(c["data"], cfg["strategy"], cfg["sampler_seed"], cfg["scale"])
    s, d, loss, grads = oracle_grads(c, smp)
    assert abs(loss - float(g["loss"])) <= 1e-3 * max(1.0, abs(float(g["loss"])))
    parity.close(s, g["src_emb"], f"{name} src_emb (autograd on)", "cawn train oracle embeddings")
    parity.close(d, g["dst_emb"], f"{name} dst_emb (autograd on)", "cawn train oracle embeddings")
    assert set(grads) == set(c["cawn_params"]) and len(grads) == 38 and all(v is not None for v in grads.values())
    assert {k.split("|")[0] for k in g if "|" in k} == set(grads)
    _check(f"cawn {name}", grads, g)
    if cfg["strategy"] != "recent":                       # the next call continues the same RandomState
        sn, nd = oracle_call(c, smp, c["src"], c["neg_dst"], c["times"])
        parity.close(sn, g["src_neg_emb"], f"{name} src_neg_emb after the gradient call", "cawn train oracle embeddings")
        parity.close(nd, g["neg_dst_emb"], f"{name} neg_dst_emb after the gradient call", "cawn train oracle embeddings")


@pytest.mark.parametrize("name", list(cc.CASES))
def test_fixture_reverse_hidden_weights_have_zero_gradient_and_bias_pairs_are_equal(name):
    """The reverse direction is read at its first step, from the zero state: weight_hh_l0_reverse gets an exactly zero gradient (a tensor,
    not None), and b_ih / b_hh enter every gate as a sum, so their gradients are the same numbers."""
    g = gc.load_golden(f"grads_cawn_{name}")
    full = lambda k: np.asarray(g[f"{k}|full"]) if f"{k}|full" in g else None
    for enc in ("feature_encoder", "position_encoder"):
        p = f"walk_encoder.{enc}.bilstm_encoder."
        k = p + "weight_hh_l0_reverse"
        if f"{k}|full" in g:
            assert not full(k).any(), k
        else:
            assert float(g[f"{k}|absmax"]) == 0.0 and not np.asarray(g[f"{k}|corner"]).any() and not np.asarray(g[f"{k}|proj"]).any(), k
        for suffix in ("", "_reverse"):
            bi, bh = full(p + "bias_ih_l0" + suffix), full(p + "bias_hh_l0" + suffix)
            # the reference's autograd sums the same terms for both, in two float32 reductions of different order: equal to summation
            # rounding (bar: a tenth of the project's gradient bar), not bit for bit; the HIP path writes one sum to both
            assert bi is not None and bh is not None and np.abs(bi).max() > 0, (enc, suffix)
            assert np.abs(bi - bh).max() <= 1e-5 * max(1.0, float(np.abs(bi).max())), (enc, suffix, float(np.abs(bi - bh).max()))


def test_oracle_dropout_sites():
    """with p = 0.5 the embeddings move, with the same seed they repeat, another seed gives others, and p = 0 is the eval forward"""
    c = cc.build_cawn_case("hub_w2_k4")
    cfg = c["cawn_cfg"]
    smp = cwo.OracleSampler(c["data"], cfg["strategy"], cfg["sampler_seed"], cfg["scale"])
    sl = dict(src=c["src"][:4], dst=c["dst"][:4], times=c["times"][:4])
    base = oracle_grads(c, smp, **sl)[0]
    e1, e2, e3 = (oracle_grads(c, smp, 0.5, s, **sl)[0] for s in (7, 7, 8))
    assert np.array_equal(e1, e2) and np.abs(e1 - e3).max() > 1e-2 and np.abs(e1 - base).max() > 1e-2
    ev = oracle_call(c, smp, sl["src"], sl["dst"], sl["times"])[0]
    assert np.array_equal(base, ev)
