#!/usr/bin/env python3
"""TCL inference step on a Wikipedia-shaped synthetic bipartite graph (8,227 + 1,000 nodes, 157,474 edges, seeded 0.5 N(0,1) node features):
B = 200 positive edges per step, K = 20 neighbours (21 positions), 2 layers, 2 heads, d = 172, `recent` sampling, sides [src ; dst ; neg_dst]
= 600 and pairs (src, dst), (src, neg_dst) = 400 per step, steps taken from the last `--span` interactions (long histories).  In ONE process,
clocks primed as bench.py's legs do:

  hip       dyglib_amd.TCL.compute_step_embeddings (sampling included), median of the timed calls, HIP events
  torch     the SAME model in plain PyTorch-ROCm ops on the same GPU: tests/tcl_oracle.py's encoder_input / layers on cuda tensors, fed the
            [n, K] neighbour arrays by this package's own device sampler (so it is not charged for a host sampler), the 400 pairs of a step
            as one batch: what a user has without the HIP path

and the largest |hip - torch| over the four results.  With `--plain` only the HIP calls run (profiling under rocprofv3 --kernel-trace --stats).
Also printed: the products the HIP kernels execute per step (flops of real rows, tile padding not counted) and the fraction of the fp32 MFMA
peak (157.3 TFLOP/s) they amount to at the measured time.  One JSON line.

    python tools/bench_tcl.py [--calls 30 --warmup 5 | --plain]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                                    # noqa: E402
from dyglib_amd import synthetic as syn                         # noqa: E402

B, K, LAYERS, HEADS, FN, FT = 200, 20, 2, 2, 172, 100
PEAK_FP32_MFMA = 157.3e12


def _stats(ms):
    ms = np.asarray(ms, dtype=np.float64)
    return {"median": round(float(np.median(ms)), 4), "min": round(float(ms.min()), 4), "p90": round(float(np.percentile(ms, 90)), 4), "calls": len(ms)}


def timed(fn, args_list, warmup):
    """HIP-event time of every call of fn over args_list (the first `warmup` untimed) -> (ms per timed call, last output)"""
    out, marks = None, []
    for i, a in enumerate(args_list):
        m0, m1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        m0.record()
        out = fn(*a)
        m1.record()
        if i >= warmup:
            marks.append((m0, m1))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in marks], out


def executed_flops(n_sides, n_pairs):
    """2 * multiply-adds of the products dygnn_tcl_forward runs for one call without taps (dyglib_amd/csrc/tcl.hip)"""
    S, d, I = K + 1, FN, 2 * n_pairs
    block = lambda rows: rows * (2 * d * d + 2 * 2 * d * 4 * d)               # out_proj + the two FFN products
    qkv = lambda seqs: seqs * S * 2 * d * 3 * d
    attn = lambda seqs, nq: seqs * nq * S * d * 2 * 2
    f = {"encode": n_sides * S * 2 * d * (FN + FN + FT), "output": I * 2 * d * d, "qkv": 0, "attention": 0, "block": 0}
    for l in range(LAYERS):
        nq = 1 if l == LAYERS - 1 else S
        n_self = n_sides if l == 0 else I
        f["qkv"] += 2 * qkv(n_self)
        f["attention"] += attn(n_self, S) + attn(I, nq)
        f["block"] += block(n_self * S) + block(I * nq)
    f["mfma_total"] = f["encode"] + f["output"] + f["qkv"] + f["block"]
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30, help="timed calls per leg (>= 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--span", type=int, default=60000, help="steps are drawn from the last SPAN interactions")
    ap.add_argument("--plain", action="store_true", help="HIP calls only (profiling)")
    a = ap.parse_args()
    from dyglib_amd import TCL, get_neighbor_sampler
    dev = "cuda:0"
    data, nf, ef = syn.make_bipartite_graph(8227, 1000, 157474, seed=0)
    nf[1:] = 0.5 * np.random.RandomState(7).standard_normal(nf[1:].shape).astype(np.float32)
    params = syn.make_tcl_params(0, K, num_layers=LAYERS)
    sampler = get_neighbor_sampler(data, "recent", seed=1, device=dev)
    model = TCL(nf, ef, sampler, FT, num_layers=LAYERS, num_heads=HEADS, num_depths=K + 1, dropout=0.1, device=dev)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    model = model.to(dev).eval()
    E = data.num_interactions
    rs, ud = np.random.RandomState(2), np.unique(data.dst_node_ids)
    n_calls = a.calls + a.warmup
    first = E - a.span

    def step(i0):
        sl = slice(i0, i0 + B)
        host = (data.src_node_ids[sl], data.dst_node_ids[sl], syn.random_negative_dst(rs, ud, B), data.node_interact_times[sl])
        return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in host)
    steps = [step(first + i * B) for i in range(n_calls)]

    def hip(s, d, ng, t):
        with torch.no_grad():
            return model.compute_step_embeddings(s, d, ng, t, num_neighbors=K)

    # ---- the same model in plain PyTorch ops on the GPU -------------------------------------------------------------------------------------
    from tests import tcl_oracle as tco
    P = {k: torch.from_numpy(v).to(dev) for k, v in params.items()}
    nf_d, ef_d = model.node_raw_features, model.edge_raw_features

    def plain(s, d, ng, t):
        with torch.no_grad():
            side = lambda roots: tco.encoder_input(P, nf_d, ef_d, roots, t, *sampler.get_historical_neighbors_device(roots, t, K))
            (ia, xa), (ib, xb), (ic, xc) = side(s), side(d), side(ng)
            oa, ob = tco.layers(P, torch.cat([ia, ia]), torch.cat([xa, xa]), torch.cat([ib, ic]), torch.cat([xb, xc]), LAYERS, HEADS)
            return oa[:B], ob[:B], oa[B:], ob[B:]

    bench._prime_gpu(dev)
    res = {}
    ms, out = timed(hip, steps, a.warmup)
    res["hip"] = {"step_ms": _stats(ms), "edges_per_s": round(B / (np.median(ms) * 1e-3), 1)}
    if not a.plain:
        bench._prime_gpu(dev)
        tms, tout = timed(plain, steps, a.warmup)
        res["torch_same_gpu"] = {"step_ms": _stats(tms), "edges_per_s": round(B / (np.median(tms) * 1e-3), 1),
                                 "what": "tests/tcl_oracle.py ops on cuda tensors, neighbour arrays from dygnn_sample_recent, 400 pairs per batch"}
        res["speedup_vs_torch"] = round(float(np.median(tms) / np.median(ms)), 2)
        res["max_abs_diff_hip_vs_torch"] = max(float((x - y).abs().max()) for x, y in zip(out, tout))
    f = executed_flops(3 * B, 2 * B)
    res["per_step"] = {"sides": 3 * B, "pairs": 2 * B, "flops": f,
                       "fraction_of_fp32_mfma_peak": round(f["mfma_total"] / (np.median(ms) * 1e-3) / PEAK_FP32_MFMA, 4)}
    res.update(metric="positive edges/s, TCL inference step (Wikipedia-shaped synthetic graph)", unit="edges/s", value=res["hip"]["edges_per_s"],
               config={"batch": B, "num_neighbors": K, "num_layers": LAYERS, "num_heads": HEADS, "sides_per_step": "[src ; dst ; neg_dst]",
                       "timer": "HIP events per call, median", "warmup_calls": a.warmup, "primed": "0.4 s of unrelated matmuls before each leg"})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
