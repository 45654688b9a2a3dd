#!/usr/bin/env python3
"""CAWN inference step on a Wikipedia-shaped synthetic bipartite graph (8,227 + 1,000 nodes, 157,474 edges, seeded 0.5 N(0,1) node features)
at the reference's Wikipedia configuration: B = 200 positive edges per step, k = 32 neighbours, walk length 1 (32 walks of 2 positions),
position_feat_dim 172, 8 walk heads (attention_dim 312), pairs (src, dst), (src, neg_dst) = 400 per step, steps taken from the last `--span`
interactions (long histories).  `--strategy recent` (default): sides [src ; dst ; neg_dst] = 600; `--strategy time_interval_aware`
(time_scaling_factor 1e-6, the reference's sampler for CAWN): the draws are replayed on the host in the reference's order, sides
[src ; dst ; src ; neg_dst] = 800.  In ONE process, clocks primed as bench.py's legs do:

  hip       dyglib_amd.CAWN.compute_step_embeddings (sampling included), median of the timed calls, HIP events
  torch     the SAME model in plain PyTorch-ROCm ops on the same GPU: tests/cawn_oracle.py's forward on cuda tensors, fed the hop arrays by
            this package's own sampler in the same order (so it is not charged for a host sampler of its own), the 400 pairs of a step as one
            batch: what a user has without the HIP path.  It already takes the two exact savings (one reverse cell, step 0 once per side).

and the largest |hip - torch| over the four results.  With `--plain` only the HIP calls run (profiling under rocprofv3 --kernel-trace --stats).
Also printed: the products the HIP kernels execute per step (flops of real rows: tile padding not counted, the flops the two savings avoid not
counted) and the fraction of the fp32 MFMA peak (157.3 TFLOP/s) they amount to at the measured time.  One JSON line, also written to `--out`.

    python tools/bench_cawn.py [--calls 30 --warmup 5 | --plain] [--strategy time_interval_aware] [--out profiles/cawn_bench.txt]
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

B, K, W, HEADS, FN, FT, PD = 200, 32, 1, 8, 172, 100, 172
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


def executed_flops(roots_a, hop_a, roots_b, hop_b):
    """2 * multiply-adds of the products dygnn_cawn_forward runs for the pairs (a_i, b_i) of one call without taps (dyglib_amd/csrc/cawn.hip);
    hop_* [pairs, k] are the hop-1 ids of the two sides"""
    n_pairs, M = hop_a.shape
    I, D = 2 * n_pairs, FN + FN + FT + PD
    A = syn.cawn_attention_dim(D, HEADS)
    R = I * M
    tree = torch.cat([roots_a.unsqueeze(1), hop_a, roots_b.unsqueeze(1), hop_b], dim=1).sort(dim=1).values
    unique = int(n_pairs + (tree[:, 1:] != tree[:, :-1]).sum().item())                 # unique node ids per pair, summed
    steps1 = int((hop_a != 0).sum().item() + (hop_b != 0).sum().item())                # valid hop-1 nodes: forward step 1 runs on these
    lstm = lambda inp, H: (I + R) * 2 * inp * 4 * H + steps1 * 2 * (inp + H) * 4 * H   # step 0 per sequence + one reverse cell per walk; step 1
    f = {"position_mlp": unique * 2 * 2 * PD * PD, "feature_lstm": lstm(D, D // 2), "position_lstm": lstm(PD, PD // 2),
         "projection_0": R * 2 * (D + PD) * A, "qkv": R * 2 * A * 3 * A, "attention": I * M * M * A * 4, "block": R * (2 * A * A + 2 * 2 * A * 4 * A),
         "output": I * 2 * A * FN}
    f["mfma_total"] = sum(v for k_, v in f.items() if k_ != "attention")
    f["not_executed"] = {"reverse_direction_beyond_one_cell": steps1 * 2 * (D + D // 2) * 4 * (D // 2) + steps1 * 2 * (PD + PD // 2) * 4 * (PD // 2),
                         "step_0_per_walk_instead_of_per_side": (R - I) * 2 * (D * 4 * (D // 2) + PD * 4 * (PD // 2))}
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30, help="timed calls per leg (>= 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--span", type=int, default=60000, help="steps are drawn from the last SPAN interactions")
    ap.add_argument("--strategy", default="recent", choices=("recent", "time_interval_aware"))
    ap.add_argument("--plain", action="store_true", help="HIP calls only (profiling)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    from dyglib_amd import CAWN, get_neighbor_sampler
    from tests import cawn_oracle as cwo
    dev = "cuda:0"
    data, nf, ef = syn.make_bipartite_graph(8227, 1000, 157474, seed=0)
    nf[1:] = 0.5 * np.random.RandomState(7).standard_normal(nf[1:].shape).astype(np.float32)
    params = syn.make_cawn_params(0, PD, W, HEADS)
    sampler = get_neighbor_sampler(data, a.strategy, time_scaling_factor=1e-6 if a.strategy != "recent" else 0.0, seed=1, device=dev)
    model = CAWN(nf, ef, sampler, FT, PD, walk_length=W, num_walk_heads=HEADS, dropout=0.1, device=dev)
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
    P = {k: torch.from_numpy(v).to(dev) for k, v in params.items()}
    nf_d, ef_d = model.node_raw_features, model.edge_raw_features
    idx = torch.arange(B, device=dev)

    def pair_sides(s, d, ng, t):
        """the sides of a step, sampled in the order compute_step_embeddings samples them, as the two sides of the 400 pairs"""
        if a.strategy == "recent":
            roots, tms, hops = model._sample([s, d, ng], t, K)
            ia, ib = torch.cat([idx, idx]), torch.cat([idx + B, idx + 2 * B])
        else:
            roots, tms, hops = model._sample([s, d, s, ng], t, K)
            ia, ib = torch.cat([idx, idx + 2 * B]), torch.cat([idx + B, idx + 3 * B])
        take = lambda i: (roots[i], [tuple(x[i] for x in h) for h in hops])
        return take(ia), take(ib), tms[ia]

    def plain(s, d, ng, t):
        with torch.no_grad():
            (ra, ha), (rb, hb), tms = pair_sides(s, d, ng, t)
            oa, ob = cwo.forward(P, nf_d, ef_d, ra, rb, tms, ha, hb, HEADS)
            return oa[:B], ob[:B], oa[B:], ob[B:]

    reset = lambda: model.set_neighbor_sampler(sampler)          # a random strategy: both legs draw the same sequence
    bench._prime_gpu(dev)
    res = {}
    reset()
    ms, out = timed(hip, steps, a.warmup)
    res["hip"] = {"step_ms": _stats(ms), "edges_per_s": round(B / (np.median(ms) * 1e-3), 1)}
    if not a.plain:
        bench._prime_gpu(dev)
        reset()
        tms, tout = timed(plain, steps, a.warmup)
        res["torch_same_gpu"] = {"step_ms": _stats(tms), "edges_per_s": round(B / (np.median(tms) * 1e-3), 1),
                                 "what": "tests/cawn_oracle.py ops on cuda tensors, hop arrays from this package's sampler, 400 pairs per batch"}
        res["speedup_vs_torch"] = round(float(np.median(tms) / np.median(ms)), 2)
        res["max_abs_diff_hip_vs_torch"] = max(float((x - y).abs().max()) for x, y in zip(out, tout))
    reset()
    with torch.no_grad():
        (ra, ha), (rb, hb), _ = pair_sides(*steps[-1])
    f = executed_flops(ra, ha[0][0], rb, hb[0][0])
    res["per_step"] = {"sides": (3 if a.strategy == "recent" else 4) * B, "pairs": 2 * B, "flops": f,
                       "fraction_of_fp32_mfma_peak": round(f["mfma_total"] / (np.median(ms) * 1e-3) / PEAK_FP32_MFMA, 4)}
    res.update(metric="positive edges/s, CAWN inference step (Wikipedia-shaped synthetic graph)", unit="edges/s", value=res["hip"]["edges_per_s"],
               config={"batch": B, "num_neighbors": K, "walk_length": W, "position_feat_dim": PD, "num_walk_heads": HEADS, "strategy": a.strategy,
                       "timer": "HIP events per call, median", "warmup_calls": a.warmup, "primed": "0.4 s of unrelated matmuls before each leg"})
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
