"""TGN training on the HIP path (dygnn_tgn_train_forward / dygnn_tgn_backward through _TgnTrainFunction): parameter gradients against the
REFERENCE's autograd (tests/golden/grads_tgn_*.npz, tools/make_golden_tgn_grads.py) and against the test-side autograd composition of the CPU
oracle off-fixture (tests/tgn_autograd.py, pinned to the same fixtures by tests/test_tgn_grads_cpu.py); the memory bank a training run leaves
against the one an inference run leaves (bit for bit); the train-mode forward against the inference forward, dropout, gradient accumulation
over the two calls of a step, finite differences, Adam, and the end-to-end example.  Bars: 1e-4 absolute for embeddings and memories,
1e-4 * max(1, max|g|) for gradients (tests/parity.py)."""
import numpy as np
import pytest
import torch

from dyglib_amd import synthetic as syn
from oracle import tgn_oracle as norc
from tests import golden_cases as gc
from tests import tgn_autograd as ta
from tests.parity import close, close_scaled
from tests.test_gradients_golden import _check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRU = "memory_updater.memory_updater."


def _model(c, strategy="recent", seed=1, tsf=0.0, dropout=0.0, train=True):
    from dyglib_amd import MemoryModel, get_neighbor_sampler
    cfg = c["tgn_cfg"]
    sampler = get_neighbor_sampler(c["data"], strategy, time_scaling_factor=tsf, seed=seed, device=DEV)
    m = MemoryModel(c["node_feat"], c["edge_feat"], sampler, time_feat_dim=cfg["time_feat_dim"], model_name="TGN", num_layers=cfg["num_layers"],
                    num_heads=cfg["num_heads"], dropout=0.1, device=DEV)
    sd = m.state_dict()
    sd.update({k: torch.from_numpy(v) for k, v in c["tgn_params"].items()})
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    m = m.train() if train else m.eval()
    m.dropout = dropout
    m.memory_bank.__init_memory_bank__()
    return m


def _calls(model, c, b, neg=True, pos=True):
    """the reference's order: negative call, then positive call"""
    k = c["tgn_cfg"]["num_neighbors"]
    out = []
    if neg:
        out += list(model.compute_src_dst_node_temporal_embeddings(b["src"], b["neg"], b["t"], edge_ids=None, edges_are_positive=False, num_neighbors=k))
    if pos:
        out += list(model.compute_src_dst_node_temporal_embeddings(b["src"], b["dst"], b["t"], edge_ids=b["eid"], edges_are_positive=True, num_neighbors=k))
    return out


def _replay(model, c, batches):
    with torch.no_grad():
        for b in batches:
            _calls(model, c, b)


def _grads(model):
    return {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters() if p.grad is not None}


def _state(model):
    mb = model.memory_bank
    return dict(node_memories=mb.node_memories.data, node_last_updated_times=mb.node_last_updated_times.data, msg=mb.msg, msg_time=mb.msg_time,
                has_msg=mb.has_msg)


def _check_fixture(name, c, g, model):
    _replay(model, c, c["tgn_batches"][:-1])
    embs = _calls(model, c, c["tgn_batches"][-1])
    for key, e in zip(("neg_src_emb", "neg_dst_emb", "pos_src_emb", "pos_dst_emb"), embs):
        close(e.detach().cpu().numpy(), g[key], f"tgn train {name} {key}")
    ta.step_loss(*embs).backward()
    got = _grads(model)
    assert sorted(got) == g["params_with_grad"].tolist()
    assert np.abs(got[GRU + "weight_ih"]).max() > 0 and np.abs(got[GRU + "weight_hh"]).max() > 0
    assert np.abs(got[GRU + "bias_ih"]).max() > 0 and np.abs(got[GRU + "bias_hh"]).max() > 0
    mb = model.memory_bank
    assert mb.node_memories.grad is None and mb.node_last_updated_times.grad is None
    assert mb.node_memories.is_leaf and not mb.node_memories.requires_grad
    _check("tgn " + name, got, g)
    close(mb.node_memories.data.cpu().numpy(), g["final_memory"], f"tgn train {name} memory")
    close(mb.node_last_updated_times.data.cpu().numpy(), g["final_last_update"], f"tgn train {name} last update")


@pytest.mark.parametrize("name", list(gc.TGN_CASES))
def test_gradients_match_reference(name):
    c = gc.build_tgn_case(name)
    _check_fixture(name, c, gc.load_golden("grads_" + name), _model(c))


def test_gradients_match_reference_uniform():
    c = gc.build_tgn_case(ta.UNIFORM_CASE)
    strategy, seed, tsf = gc.SAMPLING_STRATEGIES["uniform"]
    _check_fixture("uniform", c, gc.load_golden("grads_tgn_uniform_" + ta.UNIFORM_CASE), _model(c, strategy, seed, tsf))


@pytest.mark.parametrize("name", list(gc.TGN_CASES))
def test_training_leaves_the_memory_bank_of_inference(name):
    """two models, same weights, same batches: one runs every call under no_grad in eval mode, the other in train mode with dropout 0.1 and a
    backward per batch; the state commit does not depend on the attention, and both paths commit with the same code"""
    c = gc.build_tgn_case(name)
    ref, trn = _model(c, train=False), _model(c, dropout=0.1)
    for i, b in enumerate(c["tgn_batches"]):
        _replay(ref, c, [b])
        embs = _calls(trn, c, b)
        ta.step_loss(*embs).backward()
        trn.zero_grad()
        trn.memory_bank.detach_memory_bank()
        for key, want in _state(ref).items():
            assert torch.equal(_state(trn)[key], want), (name, i, key)


def test_train_forward_at_p0_equals_inference_and_dropout_masks():
    c = gc.build_tgn_case("tgn_gen_l2_k4")
    model = _model(c)
    _replay(model, c, c["tgn_batches"][:-1])
    backup = model.memory_bank.backup_memory_bank()
    b = c["tgn_batches"][-1]

    def run(seed=None, grad=True):
        model.memory_bank.reload_memory_bank(backup)
        model._fixed_dropout_seed = seed
        if grad:
            return torch.cat(_calls(model, c, b)).detach()
        with torch.no_grad():
            return torch.cat(_calls(model, c, b))
    close(run().cpu().numpy(), run(grad=False).cpu().numpy(), "tgn train p=0 vs inference, both call modes")
    clean = run(11)
    model.dropout = 0.1
    a, a2, other = run(11), run(11), run(12)
    assert torch.equal(a, a2)
    assert not torch.equal(a, other)
    rel = float((a - clean).norm() / clean.norm())
    assert 1e-3 < rel < 1.0, rel


def _offfixture_case(L, k, H, B, seed):
    """a bipartite graph with non-zero node features; three batches, the last one = the last interactions (users and items repeat inside
    it), its first three roots moved before every interaction (no history: all-masked attention rows); the two batches before it leave
    pending messages at some of the last batch's nodes and neighbours and none at the others"""
    data, nf, ef = syn.make_bipartite_graph(300, 60, 3000, seed=seed, time_span=2.68e6)
    nf = np.random.RandomState(seed + 1).standard_normal(nf.shape).astype(np.float32) * 0.5
    nf[0] = 0.0
    E = data.num_interactions
    rs = np.random.RandomState(seed + 3)
    uniq = np.unique(data.dst_node_ids)
    batches = []
    for lo in (E - 3 * B, E - 2 * B, E - B):
        sl = slice(lo, lo + B)
        batches.append(dict(src=data.src_node_ids[sl].copy(), dst=data.dst_node_ids[sl].copy(), t=data.node_interact_times[sl].copy(),
                            eid=data.edge_ids[sl].copy(), neg=syn.random_negative_dst(rs, uniq, B)))
    batches[-1]["t"][:3] = data.node_interact_times.min()
    return dict(data=data, node_feat=nf, edge_feat=ef, tgn_batches=batches, tgn_params=syn.make_tgn_params(seed + 2, nf.shape[0], num_layers=L),
                tgn_cfg=dict(num_layers=L, num_neighbors=k, num_heads=H, time_feat_dim=100))


@pytest.mark.parametrize("L,k,H,B", [(1, 10, 2, 200), (2, 4, 4, 24)])
def test_gradients_match_oracle_autograd(L, k, H, B):
    c = _offfixture_case(L, k, H, B, seed=50 + L)
    model = _model(c)
    _replay(model, c, c["tgn_batches"][:-1])
    last = c["tgn_batches"][-1]
    pend = model.memory_bank.has_msg.cpu().numpy()
    roots = np.unique(np.concatenate([last["src"], last["dst"], last["neg"]]))
    assert pend[roots].any() and not pend[roots].all()
    assert len(np.unique(last["src"])) < B
    embs = _calls(model, c, last)
    ta.step_loss(*embs).backward()
    got = _grads(model)
    params, _, want, _ = ta.last_batch_grads(c)
    for key, e, o in zip(("neg src", "neg dst", "pos src", "pos dst"), embs, want):
        close(e.detach().cpu().numpy(), o.detach().numpy(), f"tgn train L{L} k{k} {key} vs oracle")
    ref = {n: p.grad.numpy() for n, p in params.items() if p.grad is not None}
    assert set(got) == set(ref)
    for n in ref:
        close_scaled(got[n], ref[n], f"tgn L{L} k{k} grad {n}", label=f"tgn training gradients vs oracle autograd L{L} k{k} (scaled bar)")
        assert ((got[n] != 0) == (ref[n] != 0)).all(), (n, int(((got[n] != 0) != (ref[n] != 0)).sum()))


def _rand_loss(embs, seeds):
    return sum((e * torch.from_numpy(np.random.RandomState(s).standard_normal(tuple(e.shape)).astype(np.float32)).to(e.device)).sum()
               for e, s in zip(embs, seeds))


def test_two_calls_one_backward_sum_the_gradients():
    """the negative call's backward runs after the positive call has committed its state: it must read its own copies"""
    c = gc.build_tgn_case("tgn_bip_l1_k10")
    model = _model(c, dropout=0.1)
    model._fixed_dropout_seed = 5
    _replay(model, c, c["tgn_batches"][:-1])
    backup = model.memory_bank.backup_memory_bank()
    b = c["tgn_batches"][-1]
    res = []
    for neg, pos in ((True, True), (True, False), (False, True)):
        model.memory_bank.reload_memory_bank(backup)
        model.zero_grad()
        embs = _calls(model, c, b, neg, pos)
        _rand_loss(embs, (1, 2, 3, 4) if neg else (3, 4)).backward()
        res.append(_grads(model))
    both, g1, g2 = res
    for n in both:
        close_scaled(both[n], g1[n] + g2[n], f"tgn two calls {n}", label="tgn two calls one backward vs separate (scaled bar)")


def test_finite_differences():
    c = gc.build_tgn_case("tgn_bip_l1_k10")
    model = _model(c, dropout=0.1)
    model._fixed_dropout_seed = 11
    _replay(model, c, c["tgn_batches"][:-1])
    backup = model.memory_bank.backup_memory_bank()
    b = c["tgn_batches"][-1]

    def loss_fn():
        model.memory_bank.reload_memory_bank(backup)
        return ta.step_loss(*_calls(model, c, b))
    model.zero_grad()
    loss_fn().backward()
    torch.manual_seed(0)
    for pname, eps in ((GRU + "weight_hh", 1e-2), ("embedding_module.temporal_conv_layers.0.query_projection.weight", 1e-2)):
        target = dict(model.named_parameters())[pname]
        v = torch.randn_like(target)
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


def test_parameter_change_before_backward_and_eval_mode_raise():
    c = gc.build_tgn_case("tgn_bip_l1_k10")
    model = _model(c)
    b = c["tgn_batches"][0]
    embs = _calls(model, c, b)
    with torch.no_grad():
        model.memory_updater.memory_updater.bias_hh.add_(1.0)
    with pytest.raises(RuntimeError):
        ta.step_loss(*embs).backward()
    model.eval()
    with pytest.raises(NotImplementedError):
        _calls(model, c, b)


def test_step_embeddings_in_train_mode_are_differentiable():
    """compute_step_embeddings: one differentiable call on [positives ; negatives]; at dropout 0 its gradients are the two-call form's"""
    c = gc.build_tgn_case("tgn_bip_l1_k10")
    k = c["tgn_cfg"]["num_neighbors"]
    model = _model(c)
    _replay(model, c, c["tgn_batches"][:-1])
    backup = model.memory_bank.backup_memory_bank()
    b = c["tgn_batches"][-1]
    ta.step_loss(*_calls(model, c, b)).backward()
    two, state2 = _grads(model), {k_: v.clone() for k_, v in _state(model).items()}
    model.memory_bank.reload_memory_bank(backup)
    model.zero_grad()
    ps, pd, ns, nd = model.compute_step_embeddings(b["src"], b["dst"], b["src"], b["neg"], b["t"], b["eid"], num_neighbors=k)
    ta.step_loss(ns, nd, ps, pd).backward()
    one = _grads(model)
    for n in two:
        close_scaled(one[n], two[n], f"tgn joint step {n}", label="tgn joint step vs two calls (scaled bar)")
    for key, want in state2.items():
        assert torch.equal(_state(model)[key], want), key


def test_a_few_optimizer_steps_reduce_the_link_prediction_loss():
    """train_link_prediction.py:186-207, :242-264 in miniature: chronological batches, negative + positive call, BCE on MergeLayer logits,
    Adam, detach_memory_bank; the loss of the same batches is lower in the second pass"""
    from dyglib_amd import MergeLayer
    c = gc.build_tgn_case("tgn_bip_l1_k10")
    model = _model(c, dropout=0.1)
    merge = MergeLayer(172, 172, 172, 1)
    merge.load_state_dict({k: torch.from_numpy(v) for k, v in syn.make_merge_layer_params(7).items()})
    merge = merge.to(DEV).train()
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad] + list(merge.parameters()), lr=1e-3)
    torch.manual_seed(3)
    batches = c["tgn_batches"][:4]
    passes = []
    for _ in range(2):
        model.memory_bank.__init_memory_bank__()
        losses = []
        for b in batches:
            ns, nd, ps, pd = _calls(model, c, b)
            pos, neg = merge(ps, pd).squeeze(-1).sigmoid(), merge(ns, nd).squeeze(-1).sigmoid()
            loss = torch.nn.functional.binary_cross_entropy(torch.cat([pos, neg]), torch.cat([torch.ones_like(pos), torch.zeros_like(neg)]))
            opt.zero_grad(); loss.backward(); opt.step()
            model.memory_bank.detach_memory_bank()
            losses.append(float(loss.detach()))
        passes.append(losses)
    assert np.isfinite(passes).all() and np.mean(passes[1]) < np.mean(passes[0]), passes


def test_end_to_end_example_trains_tgn(monkeypatch):
    import importlib.util, os, sys
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "train_link_prediction_synthetic.py")
    spec = importlib.util.spec_from_file_location("train_example_tgn", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["x", "--model", "TGN", "--epochs", "2", "--users", "200", "--items", "40", "--edges", "8000", "--lr", "1e-3"])
    hist = mod.main()
    assert len(hist) == 2 and all(np.isfinite([h["train_loss"], h["val_ap"], h["val_auc"]]).all() for h in hist)
    assert hist[-1]["val_auc"] > 0.52, hist
