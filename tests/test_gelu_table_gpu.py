"""The table GELU of the fused DyGFormer inference kernels (csrc/gelu_table.h, fused3_device.h: gelu_table) on the GPU.

* The probe (dygnn_gelu_probe) stages the table into LDS by the kernels' routine at the kernels' offset and runs their device function
  (form 0), or the erf form the training kernels keep (form 1), over about 1 M arguments: a dense grid over [-8, 8], every cell edge
  +- 1 ulp, +-6 +- 1 ulp, +-0, denormals, +-1e30, +-inf and NaN.  Against float64 the table form's largest absolute error is held to twice
  that of form 1 measured by the same probe on the same finite arguments in |v| <= 8: the parent's formula is the reference, and the factor
  2 is what the embeddings' observed error of 1.5e-6 under the 1e-4 bar leaves room for sixty times over.
* The forward: 3 pairs at L = 8 / P = 2 and at L = 64 / P = 2 on the four-wave kernel, the eight-wave kernel, the packed kernel and
  tapped; 2 pairs at L = 32 / P = 1 and, on the 128-token kernel, at L = 64 / P = 1.  Every form is held to the oracle at the project's bar,
  and to the four-wave answer bit for bit: all inference instances take the table through one device function.  DYGNN_SMALL_BATCH_KERNELS
  is read once per process, so the eight-wave kernel is reached as tests/test_dygformer_large_batch_gpu.py reaches it: by a call of 257
  pairs, here the same rows over and over (rows keep their bits whatever kernel, slot or partner computes them).
* Hidden activations far beyond +-6 (the first FFN weights scaled by 50) held to the oracle: both clamps of the cell index run."""
import functools
import math

import numpy as np
import pytest
import torch

from dyglib_amd import _capi
from oracle import dygformer_oracle as orc
from tests.parity import close_scaled
from tests.test_dygformer_pack_pairs_gpu import _graph, _model, _rows

gpu = pytest.mark.gpu
DEV = "cuda:0"
CELLS = 4096
SENTINEL = -12345.0


def probe(x, form, pad=64):
    lib = _capi.load()
    n = len(x)
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)
    out = torch.full((n + pad,), SENTINEL, dtype=torch.float32, device=DEV)
    _capi.check(lib.dygnn_gelu_probe(_capi.ptr(xd), _capi.ptr(out), n, form, _capi.current_stream_ptr()))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[n:] == SENTINEL).all(), (form, n)
    return got[:n]


SPECIAL = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1.1754942e-38, -1.1754942e-38, 1e30, -1e30, np.inf, -np.inf, np.nan], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def arguments():
    f32 = np.float32
    grid = np.linspace(-8.0, 8.0, 1_000_001).astype(f32)
    edges = (-6.0 + 12.0 * np.arange(CELLS + 1) / CELLS).astype(f32)                 # exact in fp32: multiples of 3 / 1024
    around = np.concatenate([np.nextafter(edges, f32(-np.inf)), edges, np.nextafter(edges, f32(np.inf))])   # +-6 +- 1 ulp are the first and last edges'
    return np.concatenate([grid, around, SPECIAL]).astype(f32)


@gpu
def test_probe_table_form_against_float64_and_the_erf_form():
    x = arguments()
    tab, erf = probe(x, 0), probe(x, 1)
    fin = np.isfinite(x) & (np.abs(x) <= 8.0)
    x64 = torch.from_numpy(x[fin].astype(np.float64))
    exact = (0.5 * x64 * (1.0 + torch.erf(x64 / math.sqrt(2.0)))).numpy()
    e_tab, e_erf = np.abs(tab[fin].astype(np.float64) - exact), np.abs(erf[fin].astype(np.float64) - exact)
    print(f"gelu probe, {int(fin.sum())} finite arguments in |v| <= 8: max |table - exact| = {e_tab.max():.3e} at v = {x[fin][e_tab.argmax()]:.6f}, "
          f"max |erf form - exact| = {e_erf.max():.3e} at v = {x[fin][e_erf.argmax()]:.6f}")
    assert np.isfinite(tab[fin]).all()
    assert e_tab.max() <= 2.0 * e_erf.max()
    sp_t, sp_e = tab[len(x) - len(SPECIAL):], erf[len(x) - len(SPECIAL):]              # in the order of SPECIAL
    assert sp_t[0] == 0.0 and sp_t[1] == 0.0 and (np.abs(sp_t[2:8]) <= 1.2e-38).all()  # +-0, denormals, the smallest normal
    assert sp_t[8] == np.float32(1e30)
    assert sp_t[9] == 0.0 and np.signbit(sp_t[9])                                     # Phi = 0 below -6: -0, not -1e21
    assert np.array_equal(sp_t[10:12], sp_e[10:12], equal_nan=True), (sp_t[10:12], sp_e[10:12])      # +-inf: what the erf form gives
    assert np.isnan(sp_t[12])                                                         # NaN in, NaN out
    # Phi is exactly 0 at and below -6 and exactly 1 at and above +6
    lo, hi = x[fin] <= -6.0, x[fin] >= 6.0
    assert (tab[fin][lo] == 0.0).all() and np.array_equal(tab[fin][hi], x[fin][hi])


# (R_s, R_d) real tokens per side: a full pair, a pair with padding on both sides, a short one
SHAPES = {
    "L8_P2": (2, 8, [(4, 4), (1, 3), (2, 1)]),
    "L64_P2": (2, 64, [(32, 32), (7, 20), (1, 1)]),
    "L32_P1": (1, 32, [(32, 32), (5, 17)]),
    "L64_P1_128tok": (1, 64, [(64, 64), (9, 40)]),
}


@functools.lru_cache(maxsize=None)
def _reference(name):
    P, L, wanted = SHAPES[name]
    _, nf, ef, adj = _graph()[:4]
    src, dst, t = _rows(P, L, wanted)
    with torch.no_grad():
        os_, od = orc.dygformer_forward(_model(P, L)[1], nf, ef, adj, src, dst, t, P, L)
    return src, dst, t, os_.numpy(), od.numpy()


def _held(name, what, s, d):
    _, _, _, os_, od = _reference(name)
    e = max(close_scaled(s.cpu().numpy(), os_, f"table GELU {name} {what}: src emb"), close_scaled(d.cpu().numpy(), od, f"table GELU {name} {what}: dst emb"))
    print(f"{name} {what}: max |err| vs the oracle {e:.3e} (max |ref| {max(np.abs(os_).max(), np.abs(od).max()):.3g})")


@gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_on_every_inference_kernel(monkeypatch, name):
    P, L, _ = SHAPES[name]
    model = _model(P, L)[0]
    src, dst, t = _reference(name)[:3]
    B = len(src)
    with torch.no_grad():
        s4, d4 = model.compute_src_dst_node_temporal_embeddings(src, dst, t)          # small call: the four-wave kernel (one pair per workgroup where a pair is <= 64 tokens)
    _held(name, "default", s4, d4)
    # the eight-wave kernels: 257 pairs
    rep = np.arange(257) % B
    with torch.no_grad():
        s8, d8 = model.compute_src_dst_node_temporal_embeddings(src[rep], dst[rep], t[rep])
    _held(name, "257 pairs", s8[:B], d8[:B])
    assert torch.equal(s8, s4[rep]) and torch.equal(d8, d4[rep]), name
    # packed (pairs of <= 64 tokens; the 128-token shape stays where it was) and the deferred tail
    monkeypatch.setenv("DYGNN_PACK_PAIRS", "1")
    monkeypatch.setenv("DYGNN_POOLED_TAIL", "1")
    with torch.no_grad():
        sp, dp = model.compute_src_dst_node_temporal_embeddings(src, dst, t)
        sp8, dp8 = model.compute_src_dst_node_temporal_embeddings(src[rep], dst[rep], t[rep])
    monkeypatch.setenv("DYGNN_PACK_PAIRS", "0")
    with torch.no_grad():
        su, du = model.compute_src_dst_node_temporal_embeddings(src[rep], dst[rep], t[rep])      # unpacked, deferred tail
    monkeypatch.delenv("DYGNN_PACK_PAIRS")
    monkeypatch.delenv("DYGNN_POOLED_TAIL")
    _held(name, "packed", sp, dp)
    assert torch.equal(sp, s4) and torch.equal(dp, d4) and torch.equal(sp8, s8) and torch.equal(dp8, d8) and torch.equal(su, s8) and torch.equal(du, d8), name
    # tapped (the per-token last layer, PL = 2) equals untapped, on both kernel sizes
    taps = {}
    with torch.no_grad():
        st, dt = model.compute_src_dst_node_temporal_embeddings(src, dst, t, _taps=taps)
        st8, dt8 = model.compute_src_dst_node_temporal_embeddings(src[rep], dst[rep], t[rep], _taps={})
    assert len(taps["layer_outputs"]) == 2
    assert torch.equal(st, s4) and torch.equal(dt, d4) and torch.equal(st8, s8) and torch.equal(dt8, d8), name


@gpu
def test_hidden_activations_beyond_the_table_are_held_to_the_oracle():
    from dyglib_amd import DyGFormer, get_neighbor_sampler
    P, L, wanted = SHAPES["L8_P2"]
    data, nf, ef, adj = _graph()[:4]
    params = {k: v.copy() for k, v in _model(P, L)[1].items()}
    for l in range(2):
        params[f"transformers.{l}.linear_layers.0.weight"] *= np.float32(50.0)       # hidden pre-activations of std ~ 30: most lie beyond +-6
    sampler = get_neighbor_sampler(data, "recent", seed=1, device=DEV)
    model = DyGFormer(nf, ef, sampler, 100, 50, patch_size=P, num_layers=2, num_heads=2, dropout=0.1, max_input_sequence_length=L, device=DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    model = model.to(DEV).eval()
    model.impl = 3
    src, dst, t = _rows(P, L, wanted)
    with torch.no_grad():
        os_, od = orc.dygformer_forward(params, nf, ef, adj, src, dst, t, P, L)
        s, d = model.compute_src_dst_node_temporal_embeddings(src, dst, t)
    e = max(close_scaled(s.cpu().numpy(), os_.numpy(), "table GELU, ffn0 x 50: src emb"), close_scaled(d.cpu().numpy(), od.numpy(), "table GELU, ffn0 x 50: dst emb"))
    print(f"ffn0 x 50: max |err| vs the oracle {e:.3e} (max |ref| {float(max(os_.abs().max(), od.abs().max())):.3g})")
