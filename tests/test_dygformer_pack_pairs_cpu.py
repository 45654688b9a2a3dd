"""Token compaction and pair packing of the fused DyGFormer inference kernels, the parts that need no GPU.

* The packing plan (csrc/fused3_plan.h, run here on the host by the arithmetic the plan kernel runs): every pair exactly once, no
  workgroup over eight tiles or eight pairs, never more workgroups than the unpacked launch, and close to ceil(tiles / 8) on the
  headline workload's own tile counts.
* The identity the compaction rests on, in float64 on the oracle's tensors: the all-padding tokens of a pair are identical after
  every layer, and the compact forward (real tokens + one padding token, its softmax weight times its multiplicity, counted
  m_side times in the side means) is the full forward.
* The packed kernel's register budget: no scratch, no spills."""
import ctypes as C
import functools

import numpy as np
import torch

from dyglib_amd import _capi
from dyglib_amd import synthetic as syn
from oracle import dygformer_oracle as orc
from tests.parity import close
from tests.test_dygformer_resources_cpu import _resource_usage


def _lib():
    return _capi.load()


def tokens(len_s, len_d, L, P, T_s, T_d):
    """(R_s, R_d, m_s, m_d, Tc) of one pair, by the library."""
    out = (C.c_int32 * 5)()
    _lib().dygnn_dygformer_pair_tokens_host(int(len_s), int(len_d), L, P, int(T_s), int(T_d), out)
    return tuple(out)


def compact_tokens(len_s, len_d, L, P):
    """Tc per pair of ONE call (numpy): the call pads every window to its longest one."""
    ws, wd = np.minimum(len_s, L - 1) + 1, np.minimum(len_d, L - 1) + 1
    T_s, T_d = -(-ws.max() // P), -(-wd.max() // P)
    R_s, R_d = -(-ws // P), -(-wd // P)
    return R_s + R_d + ((T_s - R_s) + (T_d - R_d) > 0), T_s, T_d


def plan(tiles):
    tiles = np.ascontiguousarray(tiles, dtype=np.int32)
    wg, fw = np.empty_like(tiles), np.empty_like(tiles)
    used = _lib().dygnn_dygformer_pack_plan_host(tiles.ctypes.data, tiles.size, wg.ctypes.data, fw.ctypes.data)
    return int(used), wg, fw


def check_plan(tiles):
    tiles = np.asarray(tiles, dtype=np.int32)
    used, wg, fw = plan(tiles)
    B = tiles.size
    assert used <= (B + 1) // 2, (used, B)                       # the launch keeps the unpacked grid
    assert wg.min() >= 0 and wg.max() < used
    occupied = np.zeros((used, 8), dtype=np.int32)
    pairs = np.bincount(wg, minlength=used)
    for w, f, n in zip(wg, fw, tiles):                            # every pair appears exactly once: its waves are its own
        assert 0 <= f and f + n <= 8, (w, f, n)
        occupied[w, f:f + n] += 1
    assert occupied.max() <= 1                                     # no wave holds two pairs: <= 8 tiles per workgroup
    assert pairs.max() <= 8 and pairs.min() >= 1
    assert occupied.sum() == tiles.sum()
    return used


def test_pair_tokens_arithmetic():
    # L = 64, P = 2, call padded to 32 + 32 tokens: a window of len neighbours + the node itself
    assert tokens(0, 0, 64, 2, 32, 32) == (1, 1, 31, 31, 3)
    assert tokens(1, 2, 64, 2, 32, 32) == (1, 2, 31, 30, 4)
    assert tokens(63, 500, 64, 2, 32, 32) == (32, 32, 0, 0, 64)          # no padding at all: no padding token
    assert tokens(61, 63, 64, 2, 32, 32) == (31, 32, 1, 0, 64)
    assert tokens(9, 4, 48, 4, 5, 3) == (3, 2, 2, 1, 6)
    rs = np.random.RandomState(0)
    ls, ld = rs.randint(0, 90, 500), rs.randint(0, 90, 500)
    tc, T_s, T_d = compact_tokens(ls, ld, 64, 2)
    assert [tokens(a, b, 64, 2, T_s, T_d)[4] for a, b in zip(ls, ld)] == tc.tolist()


def test_plan_on_random_class_mixes():
    rs = np.random.RandomState(1)
    for B in (1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 31, 64, 257, 1001):
        for p in ([.25, .25, .25, .25], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [.01, .12, .34, .53], [.7, 0, .3, 0],
                  [0, .1, .9, 0], [.5, 0, 0, .5], [.05, .05, .9, 0]):
            for _ in range(3):
                check_plan(rs.choice([1, 2, 3, 4], size=B, p=p))
    for n1 in range(10):                                           # every small leftover combination
        for n2 in range(6):
            for n3 in range(4):
                for n4 in range(3):
                    if n1 + n2 + n3 + n4:
                        check_plan(rs.permutation([1] * n1 + [2] * n2 + [3] * n3 + [4] * n4))


@functools.lru_cache(maxsize=None)
def _headline_tiles():
    """Tile counts of the headline workload (bench.py: Wikipedia-shaped graph, L = 64, P = 2, the evaluation span in batches of 200,
    negatives from RandomState(2)): per evaluation batch the positive and the negative call, each padded on its own."""
    users, items, edges, L, P, B = 8227, 1000, 157474, 64, 2, 200
    data, _, _ = syn.make_bipartite_graph(users, items, edges, seed=0)
    src, dst, t = data.src_node_ids, data.dst_node_ids, data.node_interact_times
    E = data.num_interactions
    # events of a node before event i: both ends count, the graph is in time order
    ev_node = np.concatenate([src, dst])
    ev_time = np.concatenate([t, t])
    order = np.lexsort((ev_time, ev_node))
    ev_node, ev_time = ev_node[order], ev_time[order]
    start = np.searchsorted(ev_node, np.arange(ev_node.max() + 2))

    def hist(nodes, times):
        out = np.empty(nodes.size, dtype=np.int64)
        for n in np.unique(nodes):
            m = nodes == n
            out[m] = np.searchsorted(ev_time[start[n]:start[n + 1]], times[m], side="left")
        return out

    first = int(E * 0.70)
    nb = (E - first) // B
    neg_rs, uniq = np.random.RandomState(2), np.unique(dst)
    steps = []
    for i in range(nb):
        sl = slice(first + i * B, first + (i + 1) * B)
        neg = syn.random_negative_dst(neg_rs, uniq, B)
        ls = hist(src[sl], t[sl])
        calls = [compact_tokens(ls, hist(d, t[sl]), L, P) for d in (dst[sl], neg)]
        assert all(T_s == 32 and T_d == 32 for _, T_s, T_d in calls)          # every call pads to 64 tokens
        steps.append(np.concatenate([-(-tc // 16) for tc, _, _ in calls]))
    return steps


def test_plan_on_the_headline_tile_counts():
    steps = _headline_tiles()
    allt = np.concatenate(steps)
    share = np.bincount(allt, minlength=5)[1:] / allt.size
    print("tiles per pair: shares", np.round(share, 4), "mean", allt.mean())
    worst400, worst = 0.0, 0.0
    for s in steps:                                                # a single 400-pair step
        used = check_plan(s)
        worst400 = max(worst400, used / -(-int(s.sum()) // 8))
    for i in range(0, len(steps) - 31, 32):                        # 32 steps per launch: 12,800 pairs
        tiles = np.concatenate(steps[i:i + 32])
        used = check_plan(tiles)
        worst = max(worst, used / -(-int(tiles.sum()) // 8))
        print(f"launch {i // 32}: {used} workgroups, {used / (tiles.size // 2):.4f} of the unpacked launch's")
    print(f"worst used / ceil(tiles / 8): 12,800-pair launches {worst:.4f}, 400-pair steps {worst400:.4f}")
    assert worst <= 1.05 and worst400 <= 1.08


# ---- the identity, in float64 on the oracle's tensors ---------------------------------------------------------------------------
def _layer64(p, l, x, mult=None):
    """oracle/dygformer_oracle.py:encoder_layer in float64; mult[b, key] = how many identical keys a key stands for"""
    F = torch.nn.functional
    t = lambda k: torch.from_numpy(p[f"transformers.{l}." + k]).double()
    B, T, D = x.shape
    hd = D // 2
    h = F.layer_norm(x, (D,), t("norm_layers.0.weight"), t("norm_layers.0.bias"), 1e-5)
    q, k, v = F.linear(h, t("multi_head_attention.in_proj_weight"), t("multi_head_attention.in_proj_bias")).split(D, dim=-1)
    q = q.reshape(B, T, 2, hd).transpose(1, 2) * (1.0 / hd) ** 0.5
    k, v = k.reshape(B, T, 2, hd).transpose(1, 2), v.reshape(B, T, 2, hd).transpose(1, 2)
    s = q @ k.transpose(-2, -1)
    e = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    if mult is not None:
        e = e * mult[:, None, None, :]
    o = ((e / e.sum(dim=-1, keepdim=True)) @ v).transpose(1, 2).reshape(B, T, D)
    x = x + F.linear(o, t("multi_head_attention.out_proj.weight"), t("multi_head_attention.out_proj.bias"))
    h = F.gelu(F.linear(F.layer_norm(x, (D,), t("norm_layers.1.weight"), t("norm_layers.1.bias"), 1e-5), t("linear_layers.0.weight"), t("linear_layers.0.bias")))
    return x + F.linear(h, t("linear_layers.1.weight"), t("linear_layers.1.bias"))


def test_padding_tokens_are_one_token_and_the_compact_forward_is_the_full_one():
    P, L, n = 2, 64, 40
    data, nf, ef = syn.make_bipartite_graph(300, 40, 6000, seed=41)
    params = syn.make_dygformer_params(52, patch_size=P, num_layers=2)
    adj = orc.OracleAdjacency(data.src_node_ids, data.dst_node_ids, data.edge_ids, data.node_interact_times)
    idx = np.arange(2000, 2000 + n)                                # mid-graph: windows of very different lengths, much padding
    taps = {}
    with torch.no_grad():
        se, de = orc.dygformer_forward(params, nf, ef, adj, data.src_node_ids[idx], data.dst_node_ids[idx], data.node_interact_times[idx], P, L, taps=taps)
    T_s, T_d = taps["src_ids"].shape[1] // P, taps["dst_ids"].shape[1] // P
    # a patch is padding when every position of it holds node 0 (the target node sits at position 0: real tokens come first)
    pad_s = (taps["src_ids"].reshape(n, T_s, P) == 0).all(axis=2)
    pad_d = (taps["dst_ids"].reshape(n, T_d, P) == 0).all(axis=2)
    R_s, R_d = (~pad_s).sum(axis=1), (~pad_d).sum(axis=1)
    assert (pad_s[:, 1:] >= pad_s[:, :-1]).all() and (pad_d[:, 1:] >= pad_d[:, :-1]).all()
    assert (pad_s.sum() + pad_d.sum()) > n                          # the case has padding to speak of
    x0 = taps["encoder_input"].double()
    full = [x0]
    with torch.no_grad():
        for l in range(2):
            full.append(_layer64(params, l, full[-1]))
    # 1. the padding rows of a pair are identical, at the encoder input and after both layers.  float64 rounding: rows of equal input may
    #    take different summation orders inside a matrix product (~1e-16 relative per term, values <= ~20, <= 800 terms): 1e-11 is far above it
    pad = np.concatenate([pad_s, pad_d], axis=1)
    for l, x in enumerate(full):
        for b in range(n):
            rows = x[b, torch.from_numpy(pad[b])]
            if rows.shape[0] > 1:
                assert float((rows - rows[0]).abs().max()) <= 1e-11, (l, b)
    # 2. the compact forward, pair by pair
    W, bo = torch.from_numpy(params["output_layer.weight"]).double(), torch.from_numpy(params["output_layer.bias"]).double()
    worst = 0.0
    with torch.no_grad():
        for b in range(n):
            m_s, m_d = T_s - R_s[b], T_d - R_d[b]
            keep = list(range(R_s[b])) + list(range(T_s, T_s + R_d[b]))
            mult = [1.0] * len(keep)
            if m_s + m_d > 0:
                keep.append(R_s[b] if m_s > 0 else T_s + R_d[b])
                mult.append(float(m_s + m_d))
            x = x0[b:b + 1, keep]
            mu = torch.tensor([mult], dtype=torch.float64)
            for l in range(2):
                x = _layer64(params, l, x, mu)
            padrow = x[0, -1] if m_s + m_d > 0 else torch.zeros(x.shape[2], dtype=torch.float64)
            s = (x[0, :R_s[b]].sum(dim=0) + m_s * padrow) / T_s
            d = (x[0, R_s[b]:R_s[b] + R_d[b]].sum(dim=0) + m_d * padrow) / T_d
            want_s, want_d = full[2][b, :T_s].mean(dim=0), full[2][b, T_s:].mean(dim=0)
            # both are float64 forms of the same sums (<= 64 x 800 terms of magnitude <= ~20): 1e-10 is a thousand times their rounding
            worst = max(worst, float((s - want_s).abs().max()), float((d - want_d).abs().max()))
            got = torch.nn.functional.linear(torch.stack([s, d]), W, bo).float().numpy()
            close(got[0], se[b].numpy(), "compact forward in float64 vs the oracle's float32 src embedding")
            close(got[1], de[b].numpy(), "compact forward in float64 vs the oracle's float32 dst embedding")
    print("compact vs full token means, float64: max abs diff", worst)
    assert worst <= 1e-10


def test_packed_kernel_needs_no_scratch():
    usage = _resource_usage()
    hits = [v for k, v in usage.items() if "k_dygformer_fused3_packed" in k]
    assert len(hits) == 1, sorted(usage)
    print("k_dygformer_fused3_packed:", hits[0])
    assert hits[0]["ScratchSize [bytes/lane]"] == 0 and hits[0]["VGPRs Spill"] == 0, hits[0]
