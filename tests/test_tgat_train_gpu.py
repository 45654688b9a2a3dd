"""TGAT training on the HIP path (dygnn_tgat_train_forward / dygnn_tgat_backward through _TgatTrainFunction): parameter gradients against
the REFERENCE's autograd (tests/golden/grads_tgat_*.npz, tools/make_golden_tgat_grads.py) and against the CPU oracle's autograd off-fixture
(pinned to the same fixtures by tests/test_tgat_grads_cpu.py), the train-mode forward against the inference forward, dropout, gradient
accumulation over the two calls of a step, Adam, and the end-to-end example.  Bars: 1e-4 absolute for embeddings, 1e-4 * max(1, max|g|)
for gradients (tests/parity.py)."""
import numpy as np
import pytest
import torch

from dyglib_amd import synthetic as syn
from oracle import dygformer_oracle as orc
from oracle import tgat_oracle as torc
from tests import golden_cases as gc
from tests.parity import close, close_scaled
from tests.test_gradients_golden import _check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(c, strategy="recent", seed=1, tsf=0.0, dropout=0.0):
    from dyglib_amd import TGAT, get_neighbor_sampler
    cfg = c["tgat_cfg"]
    sampler = get_neighbor_sampler(c["data"], strategy, time_scaling_factor=tsf, seed=seed, device=DEV)
    m = TGAT(c["node_feat"], c["edge_feat"], sampler, time_feat_dim=cfg["time_feat_dim"], num_layers=cfg["num_layers"],
             num_heads=cfg["num_heads"], dropout=0.1, device=DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["tgat_params"].items()}, strict=True)
    m = m.to(DEV).train()
    m.dropout = dropout
    return m


def _loss(s, d, B, seeds=None):
    G1, G2 = gc.grad_loss_weights(B) if seeds is None else [np.random.RandomState(x).standard_normal((B, s.shape[1])).astype(np.float32) for x in seeds]
    return (s * torch.from_numpy(G1).to(s.device)).sum() + (d * torch.from_numpy(G2).to(d.device)).sum()


def _grads(model):
    return {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters()}


@pytest.mark.parametrize("name", list(gc.TGAT_CASES))
def test_gradients_match_reference(name):
    c = gc.build_tgat_case(name)
    g = gc.load_golden("grads_" + name)
    fwd = gc.load_golden(name)
    model = _model(c)
    s, d = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=c["tgat_cfg"]["num_neighbors"])
    close(s.detach().cpu().numpy(), fwd["src_emb"], name + " train src")
    close(d.detach().cpu().numpy(), fwd["dst_emb"], name + " train dst")
    _loss(s, d, len(c["src"])).backward()
    _check("tgat " + name, _grads(model), g)


def test_gradients_match_reference_uniform():
    name = "tgat_bip_l2_k20"
    c = gc.build_tgat_case(name)
    g = gc.load_golden("grads_tgat_uniform_" + name)
    strategy, seed, tsf = gc.SAMPLING_STRATEGIES["uniform"]
    model = _model(c, strategy, seed, tsf)
    k = c["tgat_cfg"]["num_neighbors"]
    s, d = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=k)
    close(s.detach().cpu().numpy(), g["src_emb"], "tgat uniform train src")
    close(d.detach().cpu().numpy(), g["dst_emb"], "tgat uniform train dst")
    _loss(s, d, len(c["src"])).backward()
    _check("tgat uniform", _grads(model), g)
    with torch.no_grad():                          # the next call continues the same RandomState
        ns, nd = model.compute_src_dst_node_temporal_embeddings(c["src"], c["neg_dst"], c["times"], num_neighbors=k)
    close(ns.cpu().numpy(), g["neg_src_emb"], "tgat uniform neg src")
    close(nd.cpu().numpy(), g["neg_dst_emb"], "tgat uniform neg dst")


def _offfixture_case(L, k, H, B, seed):
    """a bipartite graph with non-zero node features; the batch = the last interactions, the first three roots moved before every interaction
    (no history: all-masked attention rows)"""
    data, nf, ef = syn.make_bipartite_graph(60, 15, 1500, seed=seed, time_span=2.68e6)
    nf = np.random.RandomState(seed + 1).standard_normal(nf.shape).astype(np.float32) * 0.5
    nf[0] = 0.0
    E = data.num_interactions
    src, dst, t = data.src_node_ids[E - B:].copy(), data.dst_node_ids[E - B:].copy(), data.node_interact_times[E - B:].copy()
    t[:3] = data.node_interact_times.min()
    return dict(data=data, node_feat=nf, edge_feat=ef, src=src, dst=dst, times=t,
                tgat_params=syn.make_tgat_params(seed + 2, num_layers=L),
                tgat_cfg=dict(num_layers=L, num_neighbors=k, num_heads=H, time_feat_dim=100))


@pytest.mark.parametrize("L,k,H,B", [(3, 5, 4, 8), (2, 32, 2, 20)])
def test_gradients_match_oracle_autograd(L, k, H, B):
    c = _offfixture_case(L, k, H, B, seed=40 + L)
    model = _model(c)
    s, d = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=k)
    _loss(s, d, B, seeds=(1, 2)).backward()
    got = _grads(model)
    d_ = c["data"]
    adj = orc.OracleAdjacency(d_.src_node_ids, d_.dst_node_ids, d_.edge_ids, d_.node_interact_times)
    params = {n: torch.from_numpy(v.copy()).requires_grad_(True) for n, v in c["tgat_params"].items()}
    nf, ef = torch.from_numpy(c["node_feat"]), torch.from_numpy(c["edge_feat"])
    os_ = torc.node_embeddings(params, nf, ef, adj, c["src"], c["times"], L, k, H)
    od = torc.node_embeddings(params, nf, ef, adj, c["dst"], c["times"], L, k, H)
    close(s.detach().cpu().numpy(), os_.detach().numpy(), f"tgat train L{L} k{k} src vs oracle")
    close(d.detach().cpu().numpy(), od.detach().numpy(), f"tgat train L{L} k{k} dst vs oracle")
    _loss(os_, od, B, seeds=(1, 2)).backward()
    assert set(got) == set(params)
    for n, p in params.items():
        ref = p.grad.numpy()
        close_scaled(got[n], ref, f"tgat L{L} k{k} grad {n}", label=f"tgat training gradients vs oracle autograd L{L} k{k} (scaled bar)")
        assert ((got[n] != 0) == (ref != 0)).all(), (n, int(((got[n] != 0) != (ref != 0)).sum()))


def test_train_forward_at_p0_equals_inference():
    name = "tgat_bip_l2_k20"
    c = gc.build_tgat_case(name)
    model = _model(c)
    k = c["tgat_cfg"]["num_neighbors"]
    s, d = model.compute_src_dst_node_temporal_embeddings(c["src"], c["neg_dst"], c["times"], num_neighbors=k)
    with torch.no_grad():
        s0, d0 = model.compute_src_dst_node_temporal_embeddings(c["src"], c["neg_dst"], c["times"], num_neighbors=k)
    close(s.detach().cpu().numpy(), s0.cpu().numpy(), "tgat train p=0 vs inference src")
    close(d.detach().cpu().numpy(), d0.cpu().numpy(), "tgat train p=0 vs inference dst")


def test_dropout_masks_and_finite_differences():
    name = "tgat_bip_l2_k20"
    c = gc.build_tgat_case(name)
    model = _model(c, dropout=0.1)
    k = c["tgat_cfg"]["num_neighbors"]
    B = len(c["src"])

    def run(seed):
        model._fixed_dropout_seed = seed
        return model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=k)
    a, b = [torch.cat(run(11)).detach() for _ in range(2)]
    other = torch.cat(run(12)).detach()
    assert torch.equal(a, b)
    assert not torch.equal(a, other)
    model.dropout = 0.0
    clean = torch.cat(run(11)).detach()
    model.dropout = 0.1
    rel = float((a - clean).norm() / clean.norm())
    assert 1e-3 < rel < 1.0, rel

    def loss_fn():
        s, d = run(11)
        return _loss(s, d, B)
    model.zero_grad()
    loss_fn().backward()
    torch.manual_seed(0)
    # the time encoder's bias only along the features whose argument w dt + b stays small (w dt < 64 at the largest dt, ~2.7e6): at the
    # high frequencies one float32 ulp of the argument is up to 0.25 rad, far above any bias step, and the loss is not differentiable
    # numerically there (the analytic gradient of those features is pinned by the reference fixtures above)
    w = model.time_encoder.w.weight.detach().reshape(-1)
    low_freq = (w.abs() * 2.7e6 < 64).float()
    assert low_freq.sum() >= 10
    for pname, eps, keep in (("temporal_conv_layers.0.query_projection.weight", 1e-2, None), ("time_encoder.w.bias", 1e-2, low_freq)):
        target = dict(model.named_parameters())[pname]
        v = torch.randn_like(target)
        if keep is not None:
            v *= keep
        v /= v.norm()
        analytic = float((target.grad * v).sum())
        with torch.no_grad():
            target.add_(eps * v)
        lp = float(loss_fn().detach())
        with torch.no_grad():
            target.sub_(2 * eps * v)
        lm = float(loss_fn().detach())
        with torch.no_grad():
            target.add_(eps * v)
        numeric = (lp - lm) / (2 * eps)
        assert abs(numeric - analytic) <= 2e-2 * max(1.0, abs(analytic)), (pname, numeric, analytic)


def test_two_calls_one_backward_sum_the_gradients():
    name = "tgat_bip_l2_k20"
    c = gc.build_tgat_case(name)
    model = _model(c, dropout=0.1)
    model._fixed_dropout_seed = 5
    k = c["tgat_cfg"]["num_neighbors"]
    B = len(c["src"])

    def pos():
        s, d = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=k)
        return _loss(s, d, B, seeds=(1, 2))

    def neg():
        s, d = model.compute_src_dst_node_temporal_embeddings(c["src"], c["neg_dst"], c["times"], num_neighbors=k)
        return _loss(s, d, B, seeds=(3, 4))
    model.zero_grad()
    (pos() + neg()).backward()
    both = _grads(model)
    model.zero_grad()
    pos().backward()
    g1 = _grads(model)
    model.zero_grad()
    neg().backward()
    g2 = _grads(model)
    for n in both:
        close_scaled(both[n], g1[n] + g2[n], f"tgat two calls {n}", label="tgat two calls one backward vs separate (scaled bar)")


def test_a_few_optimizer_steps_reduce_the_link_prediction_loss():
    """train_link_prediction.py:170-185, :242-257 in miniature with TGAT: positive + negative call, BCE on MergeLayer logits, Adam."""
    from dyglib_amd import MergeLayer
    c = gc.build_tgat_case("tgat_bip_l2_k20")
    model = _model(c, dropout=0.1)
    merge = MergeLayer(172, 172, 172, 1)
    merge.load_state_dict({k: torch.from_numpy(v) for k, v in syn.make_merge_layer_params(7).items()})
    merge = merge.to(DEV).train()
    opt = torch.optim.Adam(list(model.parameters()) + list(merge.parameters()), lr=1e-3)
    k = c["tgat_cfg"]["num_neighbors"]
    losses = []
    torch.manual_seed(3)
    for _ in range(8):
        ps, pd = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=k)
        ns, nd = model.compute_src_dst_node_temporal_embeddings(c["src"], c["neg_dst"], c["times"], num_neighbors=k)
        pos, neg = merge(ps, pd).squeeze(-1).sigmoid(), merge(ns, nd).squeeze(-1).sigmoid()
        loss = torch.nn.functional.binary_cross_entropy(torch.cat([pos, neg]), torch.cat([torch.ones_like(pos), torch.zeros_like(neg)]))
        opt.zero_grad(); loss.backward(); opt.step()
        losses.append(float(loss.detach()))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses


def test_end_to_end_example_trains_tgat(monkeypatch):
    import importlib.util, os, sys
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "train_link_prediction_synthetic.py")
    spec = importlib.util.spec_from_file_location("train_example_tgat", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["x", "--model", "TGAT", "--epochs", "2", "--users", "200", "--items", "40", "--edges", "8000", "--lr", "1e-3"])
    hist = mod.main()
    assert len(hist) == 2 and all(np.isfinite([h["train_loss"], h["val_ap"], h["val_auc"]]).all() for h in hist)
    assert hist[-1]["val_auc"] > 0.52, hist
