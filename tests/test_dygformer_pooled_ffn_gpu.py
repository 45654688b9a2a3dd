"""The pooled last layer of the fused DyGFormer inference kernel.

Nothing after the last encoder layer is non-linear (models/DyGFormer.py:181-192), so the per-side token mean commutes with the last
layer's second FFN product:

    mean_tok(x_L) = mean_tok(x1) + W2 . mean_tok(gelu(h)) + b2

Inference launches take W2 after the mean.  A call whose taps ask for the last layer's per-token output runs the per-token product as
well, for the tap alone: its embeddings come from the same pooled sums and are the untapped ones bit for bit
(tests/test_dygformer_gpu.py::test_many_calls_in_one_launch_match_separate_calls compares a tapped call with an untapped launch).

Bars: embeddings 1e-4 absolute (tests/parity.py, BASELINE.json's north star), internal taps 1e-4 * max(1, max|ref|), as in
tests/test_dygformer_gpu.py.  The references are the stored fixtures of the reference implementation and oracle/dygformer_oracle.py."""
import numpy as np
import pytest
import torch

from dyglib_amd import synthetic as syn
from oracle import dygformer_oracle as orc
from tests import golden_cases as gc
from tests.parity import close, close_scaled
from tests.test_dygformer_gpu import build_model

gpu = pytest.mark.gpu


# ---- the identity itself, on the oracle's own tensors (CPU, float64) -----------------------------------------------------------
def test_pool_then_w2_equals_w2_then_pool_on_the_oracle():
    c = gc.build_case("hub_p4_l48")               # 12 tokens per side: S_src != S_dst possible, sides of unequal history
    p = c["params"]
    adj = orc.OracleAdjacency(c["data"].src_node_ids, c["data"].dst_node_ids, c["data"].edge_ids, c["data"].node_interact_times)
    taps = {}
    with torch.no_grad():
        se, de = orc.dygformer_forward(p, c["node_feat"], c["edge_feat"], adj, c["src"], c["dst"], c["times"], 4, 48, taps=taps)
    Ts = taps["src_ids"].shape[1] // 4
    x_in = taps["layer_outputs"][0].double()      # input of the last (second) layer
    t64 = lambda k: torch.from_numpy(p[k]).double()
    pre = "transformers.1."
    F = torch.nn.functional
    with torch.no_grad():
        # the last layer up to the GELU, in float64 (oracle/dygformer_oracle.py:encoder_layer)
        B, T, D = x_in.shape
        h = F.layer_norm(x_in, (D,), t64(pre + "norm_layers.0.weight"), t64(pre + "norm_layers.0.bias"), 1e-5)
        q, k, v = F.linear(h, t64(pre + "multi_head_attention.in_proj_weight"), t64(pre + "multi_head_attention.in_proj_bias")).split(D, dim=-1)
        hd = D // 2
        q = q.reshape(B, T, 2, hd).transpose(1, 2) * (1.0 / hd) ** 0.5
        k, v = k.reshape(B, T, 2, hd).transpose(1, 2), v.reshape(B, T, 2, hd).transpose(1, 2)
        o = (torch.softmax(q @ k.transpose(-2, -1), dim=-1) @ v).transpose(1, 2).reshape(B, T, D)
        x1 = x_in + F.linear(o, t64(pre + "multi_head_attention.out_proj.weight"), t64(pre + "multi_head_attention.out_proj.bias"))
        g = F.gelu(F.linear(F.layer_norm(x1, (D,), t64(pre + "norm_layers.1.weight"), t64(pre + "norm_layers.1.bias"), 1e-5),
                            t64(pre + "linear_layers.0.weight"), t64(pre + "linear_layers.0.bias")))
        W2, b2 = t64(pre + "linear_layers.1.weight"), t64(pre + "linear_layers.1.bias")
        Wo, bo = t64("output_layer.weight"), t64("output_layer.bias")
        for lo, hi, ref in ((0, Ts, se), (Ts, T, de)):
            w2_then_pool = (x1[:, lo:hi] + F.linear(g[:, lo:hi], W2, b2)).mean(dim=1)
            pool_then_w2 = x1[:, lo:hi].mean(dim=1) + F.linear(g[:, lo:hi].mean(dim=1), W2, b2)
            # float64 rounding of sums of ~12 x 800 terms of magnitude <= ~10: 1e-12 is a thousand times that
            assert float((w2_then_pool - pool_then_w2).abs().max()) < 1e-12
            # and it is the oracle's embedding (float32 arithmetic there: the parity bar)
            close(F.linear(pool_then_w2, Wo, bo).float().numpy(), ref.numpy(), "pooled form in float64 vs the oracle's float32 embedding")


# ---- every fixture of the reference ----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", list(gc.CASES))
def test_pooled_and_tapped_forms_match_the_fixtures(name):
    c = gc.build_case(name)
    g = gc.load_golden(name)
    model, _ = build_model(c)
    model.impl = 3
    taps = {}
    with torch.no_grad():
        se, de = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"])                   # pooled stream
        ts, td = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], _taps=taps)      # full stream, per-token tap
    close(se.cpu().numpy(), g["src_emb"], f"{name} pooled src emb")
    close(de.cpu().numpy(), g["dst_emb"], f"{name} pooled dst emb")
    close(ts.cpu().numpy(), g["src_emb"], f"{name} tapped src emb")
    close(td.cpu().numpy(), g["dst_emb"], f"{name} tapped dst emb")
    close(se.cpu().numpy(), ts.cpu().numpy(), f"{name} pooled vs tapped src emb")
    close(de.cpu().numpy(), td.cpu().numpy(), f"{name} pooled vs tapped dst emb")
    assert torch.equal(se, ts) and torch.equal(de, td)          # the same sums in the same order: not merely close
    S_s, S_d = g["src_pad_ids"].shape[1], g["dst_pad_ids"].shape[1]
    T = (S_s + S_d) // c["cfg"]["patch_size"]
    for l in range(2):
        close_scaled(taps["layer_outputs"][l][:gc.TAP_ROWS, :T].cpu().numpy(), g[f"layer{l}_rows"], f"{name} tapped layer {l} (internal tap, scaled bar)")


# ---- canonical sums: a row does not depend on the kernel shape, the workgroup slot or its partner ----------------------------------
@gpu
@pytest.mark.parametrize("name", ["bip_p2_l64", "hub_p4_l48"])
@pytest.mark.parametrize("B", [24, 80])           # 4 x 24 = 96 pairs: below the small-call threshold (256); 4 x 80 = 320: above it
@pytest.mark.parametrize("pos_neg", [False, True])
def test_many_rows_equal_single_calls_bit_for_bit(name, B, pos_neg):
    """The launch of N x B pairs runs four-wave workgroups (one pair each) below the threshold, eight-wave workgroups (two pairs each,
    with pos_neg_halves the positive and the negative pair of an edge) above it; the single calls always run four-wave workgroups."""
    c = gc.build_case(name)
    model, _ = build_model(c)
    model.impl = 3
    d = c["data"]
    E = d.num_interactions
    rows = [np.arange(E - 2 * B, E - B), np.arange(E - B, E)]
    rs = np.random.RandomState(11)
    src = np.stack([d.src_node_ids[r] for r in rows] * 2)
    t = np.stack([d.node_interact_times[r] for r in rows] * 2)
    dst = np.stack([d.dst_node_ids[r] for r in rows] + [rs.choice(np.unique(d.dst_node_ids), size=B) for _ in rows])
    with torch.no_grad():
        ms, md = model.compute_src_dst_node_temporal_embeddings_many(src, dst, t, pos_neg_halves=pos_neg)
        for i in range(4):
            s1, d1 = model.compute_src_dst_node_temporal_embeddings(src[i], dst[i], t[i])
            assert torch.equal(ms[i], s1) and torch.equal(md[i], d1), (name, B, pos_neg, i)


# ---- other depths, the 128-token shape, ragged sides: against the oracle ----------------------------------------------------------
def _oracle_case(users, items, edges, seed, P, L, num_layers, n, param_seed):
    from dyglib_amd import DyGFormer, get_neighbor_sampler
    data, nf, ef = syn.make_bipartite_graph(users, items, edges, seed=seed)
    params = syn.make_dygformer_params(param_seed, patch_size=P, num_layers=num_layers)
    sampler = get_neighbor_sampler(data, "recent", seed=1, device="cuda:0")
    model = DyGFormer(nf, ef, sampler, 100, 50, patch_size=P, num_layers=num_layers, num_heads=2, dropout=0.1,
                      max_input_sequence_length=L, device="cuda:0")
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    model = model.to("cuda:0").eval()
    model.impl = 3
    adj = orc.OracleAdjacency(data.src_node_ids, data.dst_node_ids, data.edge_ids, data.node_interact_times)
    idx = np.arange(data.num_interactions - n, data.num_interactions)
    src, dst, t = data.src_node_ids[idx], data.dst_node_ids[idx], data.node_interact_times[idx]
    otaps = {}
    with torch.no_grad():
        os_, od = orc.dygformer_forward(params, nf, ef, adj, src, dst, t, P, L, num_layers=num_layers, taps=otaps)
    return model, (src, dst, t), (os_.numpy(), od.numpy(), [x.numpy() for x in otaps["layer_outputs"]])


def _check_tapped_layers(taps, olayers, what):
    """Every layer's per-token output of a tapped call — the last one comes from the per-token W2 product that only the tapped form runs —
    against the oracle's, on the scaled bar of the internal taps."""
    T = olayers[0].shape[1]
    assert len(taps["layer_outputs"]) == len(olayers)
    for l, want in enumerate(olayers):
        close_scaled(taps["layer_outputs"][l][:, :T].cpu().numpy(), want, f"{what} tapped layer {l} (internal tap, scaled bar)")


@gpu
@pytest.mark.parametrize("num_layers", [1, 4])
def test_one_and_four_layers_against_oracle(num_layers):
    """num_layers = 1: the only layer is the pooled one (the stream holds no W2 block at all); 4: three per-token layers in front of it."""
    model, (src, dst, t), (os_, od, olayers) = _oracle_case(300, 40, 6000, 41, 2, 64, num_layers, 40, 50 + num_layers)
    taps = {}
    with torch.no_grad():
        gs, gd = model.compute_src_dst_node_temporal_embeddings(src, dst, t)
        ts, td = model.compute_src_dst_node_temporal_embeddings(src, dst, t, _taps=taps)
    close(gs.cpu().numpy(), os_, f"{num_layers} layers, pooled src emb")
    close(gd.cpu().numpy(), od, f"{num_layers} layers, pooled dst emb")
    assert torch.equal(gs, ts) and torch.equal(gd, td)
    _check_tapped_layers(taps, olayers, f"{num_layers} layers")


@gpu
def test_128_token_shape_against_oracle():
    """L = 512 / P = 8: one pair of up to 128 tokens per workgroup (eight token tiles per pair)."""
    model, (src, dst, t), (os_, od, olayers) = _oracle_case(6, 4, 4000, 43, 8, 512, 2, 8, 61)
    taps = {}
    with torch.no_grad():
        gs, gd = model.compute_src_dst_node_temporal_embeddings(src, dst, t)
        ts, td = model.compute_src_dst_node_temporal_embeddings(src, dst, t, _taps=taps)
    assert sum(taps["seq_lens"].cpu().tolist()) // 8 > 64          # more than four token tiles: really the 128-token kernel
    close(gs.cpu().numpy(), os_, "L=512 P=8 pooled src emb")
    close(gd.cpu().numpy(), od, "L=512 P=8 pooled dst emb")
    assert torch.equal(gs, ts) and torch.equal(gd, td)
    _check_tapped_layers(taps, olayers, "L=512 P=8")


@gpu
def test_sides_that_are_not_whole_tiles_against_oracle():
    """L = 40 / P = 2: up to 20 tokens per side, so the second token tile holds tokens of BOTH sides and the last one is partly empty."""
    model, (src, dst, t), (os_, od, olayers) = _oracle_case(60, 8, 3000, 45, 2, 40, 2, 33, 71)
    taps = {}
    with torch.no_grad():
        gs, gd = model.compute_src_dst_node_temporal_embeddings(src, dst, t)
        model.compute_src_dst_node_temporal_embeddings(src, dst, t, _taps=taps)
    S_s, S_d = taps["seq_lens"].cpu().tolist()
    assert (S_s // 2) % 16 != 0 and (S_d // 2) % 16 != 0, (S_s, S_d)
    close(gs.cpu().numpy(), os_, "L=40 P=2 pooled src emb")
    close(gd.cpu().numpy(), od, "L=40 P=2 pooled dst emb")
    _check_tapped_layers(taps, olayers, "L=40 P=2")
