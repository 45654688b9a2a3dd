"""The differentiable TCL restatement (tests/tcl_train_oracle.py) without a GPU: at p = 0 against the reference's own autograd
(tests/golden/grads_tcl_<case>.npz, written by tools/make_golden_tcl_grads.py), and a self-check of its dropout sites."""
import numpy as np
import pytest
import torch

from oracle.dropout import Drop
from tests import golden_cases as gc
from tests import parity
from tests import tcl_cases as tc
from tests import tcl_oracle as tco
from tests import tcl_train_oracle as tto
from tests.test_gradients_golden import _check
from tests.test_tcl_oracle_golden import OracleSampler


def oracle_grads(c, smp, dropout_p=0.0, seed=0):
    """(src_emb, dst_emb, loss, {name: grad}) of the fixture loss on the oracle"""
    cfg = c["tcl_cfg"]
    P = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in c["tcl_params"].items()}
    a = smp(c["src"], c["times"], cfg["K"])                 # sources first, then destinations
    b = smp(c["dst"], c["times"], cfg["K"])
    s, d = tto.tcl_train_forward(P, c["node_feat"], c["edge_feat"], c["src"], c["dst"], c["times"], a, b, cfg["layers"], cfg["heads"], dropout_p, seed)
    G1, G2 = gc.grad_loss_weights(len(c["src"]))
    loss = (s * torch.from_numpy(G1)).sum() + (d * torch.from_numpy(G2)).sum()
    loss.backward()
    return s.detach().numpy(), d.detach().numpy(), float(loss.detach()), {k: (None if p.grad is None else p.grad.numpy()) for k, p in P.items()}


@pytest.mark.parametrize("name", list(tc.CASES))
def test_oracle_autograd_matches_reference_gradients(name):
    c = tc.build_tcl_case(name)
    cfg = c["tcl_cfg"]
    g = gc.load_golden(f"grads_tcl_{name}")
    smp = OracleSampler(c["data"], cfg["strategy"], cfg["sampler_seed"])
    s, d, loss, grads = oracle_grads(c, smp)
    assert abs(loss - float(g["loss"])) <= 1e-3 * max(1.0, abs(float(g["loss"])))
    parity.close(s, g["src_emb"], f"{name} src_emb (autograd on)", "tcl train oracle embeddings")
    parity.close(d, g["dst_emb"], f"{name} dst_emb (autograd on)", "tcl train oracle embeddings")
    assert set(grads) == set(c["tcl_params"]) and all(v is not None for v in grads.values())
    assert {k.split("|")[0] for k in g if "|" in k} == set(grads)
    _check(f"tcl {name}", grads, g)
    if cfg["strategy"] != "recent":                       # the next call continues the same RandomState
        a = smp(c["src"], c["times"], cfg["K"])
        b = smp(c["neg_dst"], c["times"], cfg["K"])
        sn, nd = tco.tcl_forward(c["tcl_params"], c["node_feat"], c["edge_feat"], c["src"], c["neg_dst"], c["times"], a, b, cfg["layers"], cfg["heads"])
        parity.close(sn, g["src_neg_emb"], f"{name} src_neg_emb after the gradient call", "tcl train oracle embeddings")
        parity.close(nd, g["neg_dst_emb"], f"{name} neg_dst_emb after the gradient call", "tcl train oracle embeddings")
        assert np.abs(sn - gc.load_golden(f"tcl_{name}")["src_emb"]).max() > 1e-3      # the draws differ from a fresh sampler's


def test_oracle_dropout_sites():
    """p = 0.5: the masks of two sites and of two layers differ, each keeps half of >= 1e5 elements, kept values are doubled"""
    drop = Drop(0.5, 1234)
    n, H, S, d = 8, 2, 21, 172
    q = torch.arange(n, dtype=torch.int64)
    x = torch.ones(1)
    m0 = tto._mask(drop, 0, q, (H, S, S), x).numpy()              # layer 0 self, attention probabilities
    m2 = tto._mask(drop, 2, q, (S, 4 * d), x).numpy()             # layer 0 self, relu(fc0)
    m2_l1 = tto._mask(drop, 8 + 2, q, (S, 4 * d), x).numpy()      # layer 1 self, relu(fc0)
    m1, m3 = tto._mask(drop, 1, q, (S, d), x).numpy(), tto._mask(drop, 3, q, (S, d), x).numpy()
    assert m2.size >= 100000 and m0.size + m1.size + m3.size >= 50000
    for m in (m2, m2_l1, np.concatenate([m0.ravel(), m1.ravel(), m3.ravel(), m2.ravel()])):
        assert set(np.unique(m)) == {0.0, 2.0}                      # kept values are scaled by exactly 2
        assert abs(float((m != 0).mean()) - 0.5) <= 0.01
    assert (m2 != m2_l1).mean() > 0.4                               # layer 0 and layer 1 draw different masks
    k = min(m0.size, m2.size)
    assert (m0.ravel()[:k] != m2.ravel()[:k]).mean() > 0.4          # site 0 and site 2 draw different masks at the same element indices
    assert (m1 != m3).mean() > 0.4
    # and the forward applies them: with p = 0.5 the embeddings move, with the same seed they repeat, with p = 0 they are the eval forward
    c = tc.build_tcl_case("gen_k5_l1_h2")
    cfg = c["tcl_cfg"]
    smp = OracleSampler(c["data"], cfg["strategy"], cfg["sampler_seed"])
    base = oracle_grads(c, smp)[0]
    e1, e2, e3 = (oracle_grads(c, smp, 0.5, s)[0] for s in (7, 7, 8))
    assert np.array_equal(e1, e2) and np.abs(e1 - e3).max() > 1e-2 and np.abs(e1 - base).max() > 1e-2
    ev = tco.tcl_forward(c["tcl_params"], c["node_feat"], c["edge_feat"], c["src"], c["dst"], c["times"], smp(c["src"], c["times"], cfg["K"]),
                         smp(c["dst"], c["times"], cfg["K"]), cfg["layers"], cfg["heads"])[0]
    assert np.array_equal(base, ev)
