"""The differentiable GraphMixer restatement (tests/graphmixer_train_oracle.py) without a GPU: at p = 0 against the reference's own autograd
(tests/golden/grads_graphmixer_<case>.npz, written by tools/make_golden_graphmixer_grads.py), and a self-check of its dropout sites."""
import numpy as np
import pytest
import torch

from oracle import dygformer_oracle as orc
from oracle.dropout import Drop
from tests import golden_cases as gc
from tests import graphmixer_cases as gmc
from tests import graphmixer_oracle as gmo
from tests import graphmixer_train_oracle as gto
from tests import parity
from tests.test_gradients_golden import _check

GRAD_CASES = ("gen_k10_g7", "bip_k30_g50", "hub_k30_l3_g2000")
_CASES = {}


def case(name):
    """the recipe's inputs, built once and left unchanged"""
    if name not in _CASES:
        c = gmc.build_graphmixer_case(name)
        d = c["data"]
        c["adj"] = orc.OracleAdjacency(d.src_node_ids, d.dst_node_ids, d.edge_ids, d.node_interact_times)
        _CASES[name] = c
    return _CASES[name]


def trainable(params):
    """name -> leaf tensor; requires_grad as in the reference: everything but the frozen time encoder"""
    return {k: torch.from_numpy(v.copy()).requires_grad_(not k.startswith("time_encoder.")) for k, v in params.items()}


def oracle_grads(c, dropout_p=0.0, seed=0):
    """(src_emb, dst_emb, loss, {name: grad or None}) of the fixture loss on the oracle"""
    cfg = c["gm_cfg"]
    P = trainable(c["gm_params"])
    B = len(c["src"])
    emb = gto.graphmixer_train_forward(P, c["node_feat"], c["edge_feat"], c["adj"], np.concatenate([c["src"], c["dst"]]),
                                       np.concatenate([c["times"], c["times"]]), cfg["K"], cfg["G"], cfg["layers"], dropout_p, seed)
    G1, G2 = gc.grad_loss_weights(B)
    loss = (emb[:B] * torch.from_numpy(G1)).sum() + (emb[B:] * torch.from_numpy(G2)).sum()
    loss.backward()
    return emb[:B].detach().numpy(), emb[B:].detach().numpy(), float(loss.detach()), {k: (None if p.grad is None else p.grad.numpy()) for k, p in P.items()}


@pytest.mark.parametrize("name", GRAD_CASES)
def test_oracle_autograd_matches_reference_gradients(name):
    c = case(name)
    g = gc.load_golden(f"grads_graphmixer_{name}")
    s, d, loss, grads = oracle_grads(c)
    assert abs(loss - float(g["loss"])) <= 1e-3 * max(1.0, abs(float(g["loss"])))
    parity.close(s, g["src_emb"], f"{name} src_emb (autograd on)", "graphmixer train oracle embeddings")
    parity.close(d, g["dst_emb"], f"{name} dst_emb (autograd on)", "graphmixer train oracle embeddings")
    want = {k for k in c["gm_params"] if not k.startswith("time_encoder.")}
    assert {k for k, v in grads.items() if v is not None} == want and len(want) == len(c["gm_params"]) - 2
    assert {k.split("|")[0] for k in g if "|" in k} == want               # the reference's time encoder got no gradient either
    _check(f"graphmixer {name}", {k: grads[k] for k in want}, g)


def test_oracle_dropout_sites():
    """p = 0.5: the masks of the four sites and of two layers differ, each keeps half of >= 1e5 elements, kept values are doubled"""
    drop = Drop(0.5, 1234)
    n, K, Kh, Cc, H = 24, 30, 15, 172, 688
    q = torch.arange(n, dtype=torch.int64)
    x = torch.ones(1)
    m0 = gto._mask(drop, 0, q, (Cc, Kh), x).numpy()                # layer 0, token hidden
    m1 = gto._mask(drop, 1, q, (Cc, K), x).numpy()                 # layer 0, token FFN output
    m2 = gto._mask(drop, 2, q, (K, H), x).numpy()                  # layer 0, channel hidden
    m3 = gto._mask(drop, 3, q, (K, Cc), x).numpy()                 # layer 0, channel FFN output
    m2_l1 = gto._mask(drop, 4 + 2, q, (K, H), x).numpy()           # layer 1, channel hidden
    for m in (m1, m2, m3, m2_l1, np.concatenate([m0.ravel(), m1.ravel()])):
        assert m.size >= 100000
        assert set(np.unique(m)) == {0.0, 2.0}                       # kept values are scaled by exactly 2
        assert abs(float((m != 0).mean()) - 0.5) <= 0.01
    assert (m2 != m2_l1).mean() > 0.4                                # layer 0 and layer 1 draw different masks
    assert (m1.reshape(n, -1) != m3.reshape(n, -1)).mean() > 0.4     # two sites at the same element indices
    k = m0.size
    assert (m0.ravel() != m1.ravel()[:k]).mean() > 0.4 and (m0.ravel() != m2.ravel()[:k]).mean() > 0.4
    # the element index is q * (elements per root) + offset: a root keeps its masks wherever it stands in the list
    assert np.array_equal(gto._mask(drop, 2, q[5:7], (K, H), x).numpy(), m2[5:7])
    # and the forward applies them: with p = 0.5 the embeddings move, with the same seed they repeat, with p = 0 they are the eval forward
    c = case("gen_k10_g7")
    cfg = c["gm_cfg"]
    base = oracle_grads(c)[0]
    e1, e2, e3 = (oracle_grads(c, 0.5, s)[0] for s in (7, 7, 8))
    assert np.array_equal(e1, e2) and np.abs(e1 - e3).max() > 1e-2 and np.abs(e1 - base).max() > 1e-2
    ev = gmo.graphmixer_forward(c["gm_params"], c["node_feat"], c["edge_feat"], c["adj"], c["src"], c["times"], cfg["K"], cfg["G"], cfg["layers"])
    assert np.array_equal(base, ev)
