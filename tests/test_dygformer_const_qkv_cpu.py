"""Constant input channels of layer 0 (include/dygnn.h: DYGNN_TABLE_CONST_QKV), the parts that need no GPU.

* The tile map (csrc/fused3_plan.h: qkv_tile_row): the 38 output tiles of a layer's Q/K/V product in stream order — per head 7 q tiles,
  6 k tiles, 6 v tiles; the seventh q tile combines rows 96 .. 99 of q | k | v — held to a map written out in numpy.  Every in_proj row
  appears exactly once.
* The rank-3 operands (qkv0_const): lane (c, g) of a tile holds A | G | Bt | 0 of its row, compared with a float64 numpy formula.  The
  library sums in float64 and rounds once, so the bar is one fp32 rounding of the float64 value (2^-24 relative) plus the rounding of
  the float64 sum itself, far below it.
* The identity: with rows k < K0 of x at the bias, W[:, :K0] . LN(x)[:K0] = rs A + (-mu rs) G + Bt, in float64."""
import numpy as np
import pytest

from dyglib_amd import _capi
from dyglib_amd import synthetic as syn


def _lib():
    return _capi.load()


def numpy_tile_rows():
    """[38][16] in_proj row of every tile row, -1 for padding, written from the stream's order."""
    rows = np.full((38, 16), -1, dtype=np.int64)
    t = 0
    for h in range(2):
        for part, ntile in ((0, 7), (1, 6), (2, 6)):
            for j in range(ntile):
                if j < 6:
                    rows[t] = 200 * part + 100 * h + 16 * j + np.arange(16)
                else:                       # the combined tile: row groups 0, 1, 2 = rows 96 .. 99 of q, k, v; group 3 is padding
                    for blk in range(3):
                        rows[t, 4 * blk:4 * blk + 4] = 200 * blk + 100 * h + 96 + np.arange(4)
                t += 1
    assert t == 38
    return rows


def lib_tile_rows():
    lib = _lib()
    return np.array([[lib.dygnn_dygformer_qkv_tile_row_host(t, c) for c in range(16)] for t in range(38)], dtype=np.int64)


def test_tile_map_matches_numpy_for_both_heads_all_groups_and_the_combined_tile():
    want, got = numpy_tile_rows(), lib_tile_rows()
    assert np.array_equal(got, want)
    real = got[got >= 0]
    assert real.size == 600 and np.array_equal(np.sort(real), np.arange(600))          # every in_proj row exactly once
    for h in range(2):
        comb = got[19 * h + 6]
        assert comb.tolist() == [100 * h + 96 + r for r in range(4)] + [200 + 100 * h + 96 + r for r in range(4)] + \
            [400 + 100 * h + 96 + r for r in range(4)] + [-1] * 4
        assert got[19 * h + 7, 0] == 200 + 100 * h and got[19 * h + 13, 0] == 400 + 100 * h       # the k and the v group start here
    lib = _lib()
    assert lib.dygnn_dygformer_qkv_tile_row_host(38, 0) == -2 and lib.dygnn_dygformer_qkv_tile_row_host(0, 16) == -2
    assert lib.dygnn_dygformer_qkv_tile_row_host(-1, 0) == -2


def _weights(seed):
    p = syn.make_dygformer_params(seed, patch_size=2)
    W = np.ascontiguousarray(p["transformers.0.multi_head_attention.in_proj_weight"], dtype=np.float32)
    gamma = np.ascontiguousarray(p["transformers.0.norm_layers.0.weight"], dtype=np.float32)
    beta = np.ascontiguousarray(p["transformers.0.norm_layers.0.bias"], dtype=np.float32)
    bias = np.ascontiguousarray(np.concatenate([p["projection_layer.node.bias"], p["projection_layer.edge.bias"]]), dtype=np.float32)
    assert W.shape == (600, 200) and bias.shape == (100,)
    return W, gamma, beta, bias


def _sums64(W, gamma, beta, bias, K0):
    W64, g64, b64, x64 = (a.astype(np.float64) for a in (W, gamma, beta, bias))
    return (W64[:, :K0] * (g64[:K0] * x64[:K0])).sum(1), (W64[:, :K0] * g64[:K0]).sum(1), (W64[:, :K0] * b64[:K0]).sum(1)


@pytest.mark.parametrize("K0", [48, 96])
@pytest.mark.parametrize("seed", [0, 11])
def test_operands_hold_the_float64_sums_of_the_rows_the_map_selects(seed, K0):
    W, gamma, beta, bias = _weights(seed)
    out = np.empty((38, 64), dtype=np.float32)
    rc = _lib().dygnn_dygformer_qkv0_const_host(W.ctypes.data, gamma.ctypes.data, beta.ctypes.data, bias.ctypes.data, K0, out.ctypes.data)
    assert rc == 0
    A, G, Bt = _sums64(W, gamma, beta, bias, K0)
    rows = numpy_tile_rows()
    want = np.zeros((38, 4, 16), dtype=np.float64)           # [tile][g][c]: lane = 16 g + c
    ok = rows >= 0
    for gi, v in enumerate((A, G, Bt)):
        want[:, gi, :] = np.where(ok, v[np.where(ok, rows, 0)], 0.0)
    got = out.reshape(38, 4, 16).astype(np.float64)
    assert np.all(got[:, 3, :] == 0.0) and np.all(got[:, :3, :][~np.broadcast_to(ok[:, None, :], (38, 3, 16))] == 0.0)
    # one rounding to fp32 of a float64 sum of <= 96 terms: 2^-24 relative, plus 96 x 2^-53 of the largest partial sum
    scale = np.abs(W.astype(np.float64)[:, :K0]).sum(1).max() * max(1.0, np.abs(gamma).max() * max(1.0, np.abs(bias).max()), np.abs(beta).max())
    bar = np.abs(want) * 2.0 ** -24 + scale * 96 * 2.0 ** -53
    assert np.all(np.abs(got - want) <= bar), float(np.abs(got - want).max())
    assert np.abs(want).max() > 0


def test_bad_prefix_length_is_an_error():
    W, gamma, beta, bias = _weights(0)
    out = np.empty((38, 64), dtype=np.float32)
    assert _lib().dygnn_dygformer_qkv0_const_host(W.ctypes.data, gamma.ctypes.data, beta.ctypes.data, bias.ctypes.data, 50, out.ctypes.data) != 0


@pytest.mark.parametrize("K0", [48, 96])
def test_rank3_identity_in_float64(K0):
    W, gamma, beta, bias = _weights(11)
    rs_ = np.random.RandomState(5)
    x = rs_.standard_normal((40, 200))
    x[:, :K0] = bias[:K0].astype(np.float64)                  # the constant channels: the projection bias for every token
    mu = x.mean(1, keepdims=True)
    rs = 1.0 / np.sqrt(x.var(1, keepdims=True) + 1e-5)
    ln = (x - mu) * rs * gamma.astype(np.float64) + beta.astype(np.float64)
    full = ln[:, :K0] @ W.astype(np.float64)[:, :K0].T
    A, G, Bt = _sums64(W, gamma, beta, bias, K0)
    short = rs * A + (-mu * rs) * G + Bt
    assert np.abs(full - short).max() <= 1e-12 * max(1.0, np.abs(full).max())
