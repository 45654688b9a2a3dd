"""DyGFormer across the configurations the library accepts (tests/dygformer_config_cases.py: one row per bound of v3::supported and
train::supported and per kernel branch keyed on a dimension), against the CPU oracle:
  (a) inference by impl: 1 (generic) on every row; 3 (fused) on the fused rows, refused with NotImplementedError on the others; 0 (the
      library's choice) on every row, on fused rows also with DYGNN_PROJ_TABLES=0.  Every setting runs untapped (the launch the product
      makes: pooled tail and packed kernels included) and tapped (encoder input and every layer's output localise a failure);
  (b) training at p = 0 (eval mode, autograd on): forward and every parameter gradient vs the oracle's autograd, dispatched and, on fused
      rows, product by product (DYGNN_TRAIN_UNFUSED=1);
  (c) training at p = 0.1 with a fixed seed whose high word is live: forward and gradients vs the oracle with the training path's masks
      (oracle/dygformer_oracle.py TrainDropout, a host restatement of dropout.h), each path held to the oracle on its own; also on the
      two baseline fixtures at the default dims;
  (d) what must be refused: training at C = 64, nine layers.
Bars (tests/parity.py): 1e-4 absolute for embeddings, 1e-4 * max(1, max|ref|) for taps and gradients.  profiles/dygformer_configs.md holds
the errors observed."""
import functools

import numpy as np
import pytest
import torch

from oracle import dygformer_oracle as orc
from tests import dygformer_config_cases as cc
from tests import golden_cases as gc
from tests.parity import close, close_scaled
from tests.test_dygformer_gpu import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P_DROP = 0.1
SEED = (5 << 40) + 12345            # the seed's high word reaches the masks (key1)
IMPLS = {"generic": 1, "fused3": 3, "auto": 0}
BASELINE_ROWS = ("bip_p2_l64", "hub_p4_l48")          # golden_cases at the default dims: rows of the dropout test only

TRAINABLE = [l for l in cc.CONFIGS if l not in cc.UNTRAINABLE]
# (row, path): "unfused" = DYGNN_TRAIN_UNFUSED=1, on the rows whose dispatched path is the fused kernels
TRAIN_RUNS = [(l, path) for l in TRAINABLE for path in (("dispatched", "unfused") if l in cc.FUSED else ("dispatched",))]
DROPOUT_RUNS = TRAIN_RUNS + [(l, path) for l in BASELINE_ROWS for path in ("dispatched", "unfused")]


@functools.lru_cache(maxsize=None)
def _case(label):
    """a row of CONFIGS, a baseline fixture, or "<row>@full1": the row's graph and weights with ONE pair as the whole batch, the graph's last
    interaction whose two nodes both have at least L - 1 earlier interactions (both windows full)"""
    if label.endswith("@full1"):
        row = label[:-len("@full1")]
        c = dict(cc.build(row))
        g, L = c["data"], cc.dims(row)["L"]
        for i in range(g.num_interactions - 1, -1, -1):
            before = g.node_interact_times < g.node_interact_times[i]
            if all(int((((g.src_node_ids == n) | (g.dst_node_ids == n)) & before).sum()) >= L - 1 for n in (g.src_node_ids[i], g.dst_node_ids[i])):
                break
        c.update(src=g.src_node_ids[i:i + 1].copy(), dst=g.dst_node_ids[i:i + 1].copy(), neg_dst=g.dst_node_ids[i:i + 1].copy(),
                 times=g.node_interact_times[i:i + 1].copy())
        return c
    return cc.build(label) if label in cc.CONFIGS else gc.build_case(label)


def _oracle_forward(label, params, **kw):
    c = _case(label)
    cfg, g = c["cfg"], c["data"]
    adj = orc.OracleAdjacency(g.src_node_ids, g.dst_node_ids, g.edge_ids, g.node_interact_times)
    return orc.dygformer_forward(params, c["node_feat"], c["edge_feat"], adj, c["src"], c["dst"], c["times"], cfg["patch_size"],
                                 cfg["max_input_sequence_length"], cfg["num_heads"], cfg["num_layers"], **kw)


@functools.lru_cache(maxsize=None)
def _oracle_inference(label):
    taps = {}
    with torch.no_grad():
        s, d = _oracle_forward(label, _case(label)["params"], taps=taps)
    return s.numpy(), d.numpy(), taps


def _loss_weights(label):
    c = _case(label)
    B, Fn = len(c["src"]), c["node_feat"].shape[1]
    return [torch.from_numpy(np.random.RandomState(x).standard_normal((B, Fn)).astype(np.float32)) for x in (1, 2)]


@functools.lru_cache(maxsize=None)
def _oracle_training(label, p):
    """embeddings and parameter gradients of L = sum(src * G1) + sum(dst * G2) by autograd through the oracle; p > 0: with the training
    path's masks"""
    params = {n: torch.from_numpy(v.copy()).requires_grad_(True) for n, v in _case(label)["params"].items()}
    s, d = _oracle_forward(label, params, dropout=orc.TrainDropout(p, SEED) if p > 0 else None)
    G1, G2 = _loss_weights(label)
    ((s * G1).sum() + (d * G2).sum()).backward()
    return s.detach().numpy(), d.detach().numpy(), {n: v.grad.numpy() for n, v in params.items()}


def _setenv(monkeypatch, env):
    for name in ("DYGNN_PROJ_TABLES", "DYGNN_POOLED_TAIL", "DYGNN_PACK_PAIRS", "DYGNN_TRAIN_UNFUSED", "DYGNN_CONST_QKV"):
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        monkeypatch.setenv(name, val)


@pytest.mark.parametrize("impl", list(IMPLS))
@pytest.mark.parametrize("label", list(cc.CONFIGS))
def test_inference_against_oracle(label, impl, monkeypatch):
    d, c = cc.dims(label), cc.build(label)
    model, _ = build_model(c)
    model.impl = IMPLS[impl]
    _setenv(monkeypatch, d["env"])
    if impl == "fused3" and label not in cc.FUSED:
        with pytest.raises(NotImplementedError), torch.no_grad():          # DYGNN_E_UNSUPPORTED from host code, before any launch
            model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"])
        return
    os_, od, otaps = _oracle_inference(label)
    S_s, S_d = cc.PADDED[label]
    T = (S_s + S_d) // d["P"]
    settings = [{}]
    if impl == "auto" and label in cc.FUSED:
        settings.append({"DYGNN_PROJ_TABLES": "0"})
    if impl != "generic":
        settings += list(cc.EXTRA_ENV.get(label, ()))
    for env in settings:
        _setenv(monkeypatch, dict(d["env"], **env))
        how = impl + "".join(f" {k}={v}" for k, v in env.items())
        tag = f"dygformer configs {label}: inference {how}"
        taps = {}
        with torch.no_grad():
            s, t = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"])
            ts, tt = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], _taps=taps)
        assert s.shape == (d["B"], d["Fn"]) and s.dtype == torch.float32
        assert taps["seq_lens"].cpu().tolist() == [S_s, S_d]
        # the taps first: the earliest stage that is off names the kernel code to read
        close_scaled(taps["encoder_input"][:, :T].cpu().numpy(), otaps["encoder_input"].numpy(), f"{tag} encoder input", label=f"{tag}, taps (scaled bar)")
        for l in range(d["NL"]):
            close_scaled(taps["layer_outputs"][l][:, :T].cpu().numpy(), otaps["layer_outputs"][l].numpy(), f"{tag} layer {l}", label=f"{tag}, taps (scaled bar)")
        for got, want, what in ((ts, os_, "tapped src"), (tt, od, "tapped dst"), (s, os_, "src"), (t, od, "dst")):
            close(got.cpu().numpy(), want, f"{tag} {what} emb", label=f"{tag}, embeddings")


def _train_and_compare(label, path, p, monkeypatch):
    c = _case(label)
    model, _ = build_model(c)
    _setenv(monkeypatch, {"DYGNN_TRAIN_UNFUSED": "1"} if path == "unfused" else {})
    if p > 0:
        model.train()
        model.dropout = p
    else:
        model.eval()                                   # dropout off, autograd on: the training kernels with p = 0
    model._fixed_dropout_seed = SEED
    s, t = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"])
    assert s.requires_grad and t.requires_grad
    G1, G2 = (g.to(DEV) for g in _loss_weights(label))
    ((s * G1).sum() + (t * G2).sum()).backward()
    got = {n: v.grad.detach().cpu().numpy() for n, v in model.named_parameters()}
    os_, od, ref = _oracle_training(label, p)
    tag = f"dygformer configs {label}: training p={p:g} {path}"
    close(s.detach().cpu().numpy(), os_, f"{tag} src emb", label=f"{tag}, embeddings")
    close(t.detach().cpu().numpy(), od, f"{tag} dst emb", label=f"{tag}, embeddings")
    assert set(got) == set(ref)
    for n in ref:
        close_scaled(got[n], ref[n], f"{tag} grad {n}", label=f"{tag}, gradients (scaled bar)")
        assert bool(got[n].any()) == bool(ref[n].any()), (n, "all-zero gradient on one side only")
    return s.detach()


@pytest.mark.parametrize("label,path", TRAIN_RUNS)
def test_training_without_dropout_against_oracle_autograd(label, path, monkeypatch):
    _train_and_compare(label, path, 0.0, monkeypatch)


@pytest.mark.parametrize("label,path", DROPOUT_RUNS)
def test_training_with_dropout_against_oracle_autograd(label, path, monkeypatch):
    """Masks are integer comparisons (hash >= threshold): no element is borderline, none is excluded."""
    s = _train_and_compare(label, path, P_DROP, monkeypatch)
    plain = _oracle_training(label, 0.0)[0]
    assert float(np.abs(s.cpu().numpy() - plain).max()) > 1e-3           # the masks did something


@pytest.mark.parametrize("label,path", [("ft18", "dispatched"), ("two_pair_f32", "dispatched"), ("two_pair_f32", "unfused")])
def test_training_a_single_pair_with_full_windows(label, path, monkeypatch):
    """B = 1 with both windows full: the one shape at which the workspace's dPc block (B S rows of C floats, a whole number of 256-byte
    units at these rows) is smaller than the dh table [S + 1][C] the co-occurrence backward keeps in it.  The table's last row once
    ran over the next block, dlut, while that was being read: its count-0 row, so the co-occurrence encoder's gradients were wrong."""
    c = _case(label + "@full1")
    d = cc.dims(label)
    assert len(c["src"]) == 1 and (2 * d["L"] * d["C"] * 4) % 256 == 0 and d["L"] % d["P"] == 0
    taps = {}
    with torch.no_grad():
        _oracle_forward(label + "@full1", c["params"], taps=taps)
    assert taps["src_ids"].shape[1] == taps["dst_ids"].shape[1] == d["L"]
    _train_and_compare(label + "@full1", path, 0.0, monkeypatch)


@pytest.mark.parametrize("label", list(cc.UNTRAINABLE))
def test_untrainable_row_refuses_gradients_and_still_infers(label):
    c = cc.build(label)
    model, _ = build_model(c)
    with pytest.raises(NotImplementedError):
        model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"])          # eval mode, autograd recording
    model.train()
    with pytest.raises(NotImplementedError):
        model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"])
    model.eval()
    os_, od, _ = _oracle_inference(label)
    with torch.no_grad():
        s, t = model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"])
    tag = f"dygformer configs {label}: inference after a refused training call"
    close(s.cpu().numpy(), os_, f"{tag} src emb", label=tag)
    close(t.cpu().numpy(), od, f"{tag} dst emb", label=tag)


def test_nine_layers_are_refused_before_any_launch():
    c = cc.build(cc.NINE_LAYERS, 9)
    model, _ = build_model(c)
    assert len(model.transformers) == 9
    with pytest.raises(AssertionError, match="num_layers"), torch.no_grad():
        model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"])
    with pytest.raises(AssertionError, match="num_layers"):
        model.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"])          # the training entry too
