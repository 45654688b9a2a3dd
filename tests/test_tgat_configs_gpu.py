"""TGAT across the configurations the library accepts (check_tgat: dims multiples of 4, L in 1..3, head dim a multiple of 4, k <= 64,
Dq = Fn + Ft <= 272, Dkv = Fn + Fe + Ft <= 1024), one row of CONFIGS per path boundary of the kernels, against the CPU oracle:
  (a) inference, layers as GEMMs;  (b) inference, layers as row-block chains (DYGNN_TGAT_CHAIN=1; the GEMM form again where chain::fits
  does not hold);  (c) training at p = 0: forward and parameter gradients vs the oracle's autograd;  (d) training at p = 0.1 with a fixed
  seed: forward and gradients vs the oracle with the training path's dropout masks (oracle/dropout.py, a host copy of dropout.h).
Bars: 1e-4 absolute for embeddings, 1e-4 * max(1, max|g|) for gradients (tests/parity.py)."""
import functools

import numpy as np
import pytest
import torch

from dyglib_amd import synthetic as syn
from oracle import dygformer_oracle as orc
from oracle import tgat_oracle as torc
from tests.parity import close, close_scaled

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P_DROP = 0.1
SEED = (5 << 40) + 12345            # the seed's high word reaches the masks (key1)

# label: (Fn, Fe, Ft, H, k, L, B, env) -- what each one crosses
CONFIGS = {
    # Dq = 32 < 48 at levels of >= 48 rows: the query product cannot gather its rows (LDS-DMA GEMM needs N >= 48); training GEMMs with N < 48
    "dq32": (16, 8, 16, 2, 10, 2, 30, {}),
    # the smallest head dim (4), Dkv = 12, three layers
    "dims4_l3": (4, 4, 4, 2, 3, 3, 10, {}),
    # one head (head dim = Dq = 64), k = 7 (idle row slots)
    "h1": (40, 24, 24, 1, 7, 2, 20, {}),
    # H > 2 (k_tgat_attn_lin<20, 2>); 4 + 2 H = 20 weight-gradient problems: two dw_grouped launches
    "h8_k20": (100, 172, 28, 8, 20, 2, 12, {}),
    # Dkv = 616 > 512: inference attention with four float4 columns per lane; training columns in lane slot u = 2
    "dkv616": (172, 344, 100, 2, 10, 1, 40, {}),
    # Dkv = 1024, the bound of both paths; k > 20 (k_tgat_attn_lin<0, *>)
    "dkv1024_k24": (172, 752, 100, 2, 24, 1, 8, {}),
    # just past the two-wave attention kernel (k = 21)
    "k21": (172, 172, 100, 2, 21, 2, 6, {}),
    # the largest H and k: 68 heads of 4 (more heads than lanes in the softmax), LDS of k_tgat_attn_lin<0, 2> above 64 KiB; pairs[] full
    "h68_k64": (172, 172, 100, 68, 64, 1, 4, {}),
    # the largest Ft with H > 2: LDS of k_tgat_attn_lin<20, 2> above 64 KiB (85 KiB)
    "ft268_h4": (4, 172, 268, 4, 20, 1, 20, {}),
    # k = 1, three layers
    "k1_l3": (172, 172, 100, 2, 1, 3, 25, {}),
    # one pair: two rows at the top level
    "b1": (172, 172, 100, 2, 20, 2, 1, {}),
    # the general GEMM without LDS-DMA (documented A/B switch, read per call): the query product of levels >= 48 rows must not gather its rows
    "mm_dma0": (172, 172, 100, 2, 10, 2, 10, {"DYGNN_MM_DMA": "0"}),
}


@functools.lru_cache(maxsize=None)
def _case(label):
    """a bipartite graph (75 nodes, 1500 edges) with non-zero node features; the batch = the last B interactions, the first three roots
    moved before every interaction (no history: all-masked attention rows)"""
    Fn, Fe, Ft, H, k, L, B, _ = CONFIGS[label]
    seed = 50 + sorted(CONFIGS).index(label)
    data, _, ef = syn.make_bipartite_graph(60, 15, 1500, seed=seed, time_span=2.68e6, edge_feat_dim=Fe)
    nf = np.random.RandomState(seed + 1).standard_normal((data.max_node_id + 1, Fn)).astype(np.float32) * 0.5
    nf[0] = 0.0
    E = data.num_interactions
    src, dst, t = data.src_node_ids[E - B:].copy(), data.dst_node_ids[E - B:].copy(), data.node_interact_times[E - B:].copy()
    t[:3] = data.node_interact_times.min()
    params = syn.make_tgat_params(seed + 2, node_feat_dim=Fn, edge_feat_dim=Fe, time_feat_dim=Ft, num_layers=L)
    adj = orc.OracleAdjacency(data.src_node_ids, data.dst_node_ids, data.edge_ids, data.node_interact_times)
    return dict(data=data, nf=nf, ef=ef, src=src, dst=dst, t=t, params=params, adj=adj)


def _loss_weights(B, Fn):
    return [torch.from_numpy(np.random.RandomState(x).standard_normal((B, Fn)).astype(np.float32)) for x in (1, 2)]


@functools.lru_cache(maxsize=None)
def _oracle(label, p):
    """embeddings and parameter gradients of the oracle: p = 0 the plain oracle on src and on dst; p > 0 the training path's layout, one
    call on [src ; dst] at [t ; t] with its masks"""
    Fn, Fe, Ft, H, k, L, B, _ = CONFIGS[label]
    c = _case(label)
    params = {n: torch.from_numpy(v.copy()).requires_grad_(True) for n, v in c["params"].items()}
    nf, ef = torch.from_numpy(c["nf"]), torch.from_numpy(c["ef"])
    if p == 0:
        s = torc.node_embeddings(params, nf, ef, c["adj"], c["src"], c["t"], L, k, H)
        d = torc.node_embeddings(params, nf, ef, c["adj"], c["dst"], c["t"], L, k, H)
    else:
        both = torc.node_embeddings(params, nf, ef, c["adj"], np.concatenate([c["src"], c["dst"]]), np.concatenate([c["t"], c["t"]]), L, k, H,
                                    dropout=torc.TrainDropout(p, SEED))
        s, d = both[:B], both[B:]
    G1, G2 = _loss_weights(B, Fn)
    ((s * G1).sum() + (d * G2).sum()).backward()
    return s.detach().numpy(), d.detach().numpy(), {n: v.grad.numpy() for n, v in params.items()}


def _model(label, train, p=0.0):
    from dyglib_amd import TGAT, get_neighbor_sampler
    Fn, Fe, Ft, H, k, L, B, _ = CONFIGS[label]
    c = _case(label)
    sampler = get_neighbor_sampler(c["data"], "recent", seed=1, device=DEV)
    m = TGAT(c["nf"], c["ef"], sampler, Ft, num_layers=L, num_heads=H, dropout=0.1, device=DEV)
    m.load_state_dict({n: torch.from_numpy(v) for n, v in c["params"].items()}, strict=True)
    m = m.to(DEV)
    m.train(train)
    m.dropout = p
    m._fixed_dropout_seed = SEED
    return m


def _env(label, monkeypatch):
    for name, val in CONFIGS[label][7].items():
        monkeypatch.setenv(name, val)


@pytest.mark.parametrize("form", ["gemm", "chains"])
@pytest.mark.parametrize("label", list(CONFIGS))
def test_inference_against_oracle(label, form, monkeypatch):
    Fn, Fe, Ft, H, k, L, B, _ = CONFIGS[label]
    c = _case(label)
    m = _model(label, train=False)
    _env(label, monkeypatch)
    monkeypatch.setenv("DYGNN_TGAT_CHAIN", "1" if form == "chains" else "0")
    with torch.no_grad():
        s, d = m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["t"], num_neighbors=k)
    os_, od, _ = _oracle(label, 0.0)
    close(s.cpu().numpy(), os_, f"{label} inference ({form}) src", label=f"configs {label}: inference ({form})")
    close(d.cpu().numpy(), od, f"{label} inference ({form}) dst", label=f"configs {label}: inference ({form})")


@pytest.mark.parametrize("p", [0.0, P_DROP], ids=["p0", "dropout"])
@pytest.mark.parametrize("label", list(CONFIGS))
def test_training_against_oracle_autograd(label, p, monkeypatch):
    Fn, Fe, Ft, H, k, L, B, _ = CONFIGS[label]
    c = _case(label)
    m = _model(label, train=True, p=p)
    _env(label, monkeypatch)
    s, d = m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["t"], num_neighbors=k)
    G1, G2 = (g.to(DEV) for g in _loss_weights(B, Fn))
    ((s * G1).sum() + (d * G2).sum()).backward()
    got = {n: v.grad.detach().cpu().numpy() for n, v in m.named_parameters()}
    os_, od, ref = _oracle(label, p)
    tag = f"configs {label}: training p={p:g}"
    close(s.detach().cpu().numpy(), os_, f"{tag} src", label=f"{tag} forward")
    close(d.detach().cpu().numpy(), od, f"{tag} dst", label=f"{tag} forward")
    assert set(got) == set(ref)
    for n in ref:
        close_scaled(got[n], ref[n], f"{tag} grad {n}", label=f"{tag} gradients (scaled bar)")
        if p == 0:
            assert ((got[n] != 0) == (ref[n] != 0)).all(), (n, int(((got[n] != 0) != (ref[n] != 0)).sum()))
