"""Training path above 256 pairs: the eight-wave, two-pairs-per-workgroup instances k_dygformer_fused3<4, true, 8>, k_attn_bwd<4, 8> and
k_ffn_bwd<8> (dispatch: dygformer_fused3_train.hip, dygformer_fused3_bwd.hip) — the kernels of a batch-200 training step through
compute_src_dst_node_temporal_embeddings_many and of bench.py's training leg, which no gradient test below B = 40 reaches.

Recipes: tests/large_batch_cases.py (odd B: the last workgroup holds one pair; dense row counts that leave k_ffn_bwd<8>'s last workgroup
half full / its last active wave half valid; T = 14 on k_attn_bwd's scalar path with the four-wave FFN backward behind an eight-wave
forward).  The bars are the project's own (tests/parity.py): embeddings plain 1e-4, gradients 1e-4 * max(1, max|reference|), against torch
autograd through the CPU oracle — the harness of tests/test_train_gpu.py, itself pinned to the reference's gradient fixtures by
test_oracle_autograd_matches_reference_gradients."""
import numpy as np
import pytest
import torch

from dyglib_amd import synthetic as syn
from tests import large_batch_cases as lb
from tests.parity import close, close_scaled
from tests.test_dygformer_gpu import build_model
from tests.test_train_gpu import _loss_weights, _oracle_grads

pytestmark = pytest.mark.gpu


def _check_against_oracle(c, tag):
    model, _ = build_model(c)
    G1, G2 = _loss_weights(c)
    want, ws, wd = _oracle_grads(c, G1, G2)
    model.eval()                                   # dropout off, autograd on: the training kernels with p = 0
    for p in model.parameters():
        p.grad = None
    s, t = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"])
    assert s.requires_grad and t.requires_grad
    for got, ref, side in ((s, ws, "src"), (t, wd, "dst")):
        close(got.detach().cpu().numpy(), ref, f"train forward {tag} {side} emb", label=f"eight-wave training forward vs oracle, {tag}, {side} emb")
    ((s * torch.from_numpy(G1).cuda()).sum() + (t * torch.from_numpy(G2).cuda()).sum()).backward()
    names = [k for k, _ in model.named_parameters()]
    assert sorted(names) == sorted(want)
    for k, p in model.named_parameters():
        got = p.grad.detach().cpu().numpy()
        assert got.shape == want[k].shape, k
        assert (float(np.abs(got).max()) > 0) == (float(np.abs(want[k]).max()) > 0), k          # no tensor's gradient went missing, none appeared
        close_scaled(got, want[k], f"{tag} grad {k}", label=f"eight-wave gradient vs oracle autograd, {tag}: {k}")
    return want


@pytest.mark.parametrize("name", ["full64", "ragged40", "hub14"])
def test_gradients_match_oracle_autograd(name):
    c = lb.build(name)
    want = _check_against_oracle(c, name)
    if name != "hub14":          # non-zero node features: the node projection really has a gradient to get wrong
        assert float(np.abs(want["projection_layer.node.weight"]).max()) > 0


def test_four_layers_at_257_pairs():
    """20 grouped weight-gradient problems (4 per encoder layer + 4 projections) fed by eight-wave activations."""
    c = lb.build("full64", num_layers=4, params=syn.make_dygformer_params(77, patch_size=2, num_layers=4))
    _check_against_oracle(c, "full64, 4 layers")


@pytest.mark.parametrize("name", ["full64", "hub14"])
def test_fused_matches_product_by_product_with_dropout(name, monkeypatch):
    """Train mode, masks pinned: the fused kernels and the product-by-product path (DYGNN_TRAIN_UNFUSED=1, read by the library on every call)
    draw their masks from the same counter-based hash of the DENSE row and column.  A two-pair kernel that hashed its workgroup slot instead
    of the row it owns would agree with itself and disagree here."""
    c = lb.build(name)
    model, _ = build_model(c)
    model.train()
    assert model.dropout == 0.1
    model._fixed_dropout_seed = 4321
    G1, G2 = (torch.from_numpy(g).cuda() for g in _loss_weights(c))

    def run():
        for p in model.parameters():
            p.grad = None
        s, t = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"])
        ((s * G1).sum() + (t * G2).sum()).backward()
        return s.detach().clone(), t.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    fs, ft, fg = run()
    monkeypatch.setenv("DYGNN_TRAIN_UNFUSED", "1")
    us, ut, ug = run()
    monkeypatch.delenv("DYGNN_TRAIN_UNFUSED")
    assert bool(fs.any()) and bool(ft.any())
    with torch.no_grad():
        model.eval()
        es, _ = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"])
    assert float((fs - es).norm() / es.norm()) > 1e-3          # the masks were on
    emb = f"eight-wave fused vs product-by-product (dropout on), {name}, "
    close(fs.cpu().numpy(), us.cpu().numpy(), f"fused vs unfused train forward {name} src", label=emb + "src emb")
    close(ft.cpu().numpy(), ut.cpu().numpy(), f"fused vs unfused train forward {name} dst", label=emb + "dst emb")
    for k in fg:
        close_scaled(fg[k].cpu().numpy(), ug[k].cpu().numpy(), f"fused vs unfused grad {name} {k}",
                     label=f"eight-wave fused vs product-by-product (dropout on), {name}, gradient: {k}")


def test_dropout_is_seeded_at_257_pairs():
    c = lb.build("full64")
    model, _ = build_model(c)
    model.train()
    outs = []
    for seed in (1234, 1234, 99):
        model._fixed_dropout_seed = seed
        s, t = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"])
        outs.append((s.detach(), t.detach()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])          # same seed, same masks
    assert not torch.equal(outs[0][0], outs[2][0]) and not torch.equal(outs[0][1], outs[2][1])
    # the lone pair of the half-full last workgroup draws masks too
    assert not torch.equal(outs[0][0][-1], outs[2][0][-1])


def test_one_pass_of_two_calls_equals_two_small_calls():
    """The shape bench.py's training leg times: [positives ; negatives] of 200 pairs each as ONE dense pass of 400 pairs (eight-wave
    kernels) against the two 200-pair calls made separately (four-wave kernels)."""
    c = lb.build("full64")
    d = c["data"]
    E, B = d.num_interactions, 200
    idx = np.arange(E - B, E)
    src, dst, t = d.src_node_ids[idx], d.dst_node_ids[idx], d.node_interact_times[idx]
    neg = syn.random_negative_dst(np.random.RandomState(8), np.unique(d.dst_node_ids), B)
    model, _ = build_model(c)
    model.eval()                                   # dropout off, autograd on
    rs = np.random.RandomState(5)
    G = [torch.from_numpy(rs.standard_normal((B, 172)).astype(np.float32)).cuda() for _ in range(4)]
    host = [np.stack([src, src]), np.stack([dst, neg]), np.stack([t, t])]
    devt = [torch.from_numpy(x).cuda() for x in host]
    lens = model._seq_lens_groups(*host, *devt, torch.device("cuda:0"))
    assert lens == [(64, 64), (64, 64)], lens          # equal: _many runs one pass over 400 pairs

    def loss_of(ps, pd, ns, nd):
        return (ps * G[0]).sum() + (pd * G[1]).sum() + (ns * G[2]).sum() + (nd * G[3]).sum()

    for p in model.parameters():
        p.grad = None
    ps, pd = model.compute_src_dst_node_temporal_embeddings(src, dst, t)
    ns, nd = model.compute_src_dst_node_temporal_embeddings(src, neg, t)
    loss_of(ps, pd, ns, nd).backward()
    want = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    for p in model.parameters():
        p.grad = None
    s, dd = model.compute_src_dst_node_temporal_embeddings_many(*host)
    assert s.shape == (2, B, 172) and s.requires_grad
    for what, got, ref in (("pos src", s[0], ps), ("pos dst", dd[0], pd), ("neg src", s[1], ns), ("neg dst", dd[1], nd)):
        err, bar = float((got - ref).detach().abs().max()), 1e-6 * max(1.0, float(ref.detach().abs().max()))
        print(f"one pass of 400 vs two calls of 200, {what} emb: max|err| {err:.3e} (bar {bar:.1e})")
        assert err <= bar, (what, err, bar)
    loss_of(s[0], dd[0], s[1], dd[1]).backward()
    for k, p in model.named_parameters():
        close_scaled(p.grad.cpu().numpy(), want[k].cpu().numpy(), f"one pass of 400 vs two calls of 200, grad {k}",
                     label=f"one eight-wave pass of 400 pairs vs two four-wave calls of 200, gradient: {k}")
