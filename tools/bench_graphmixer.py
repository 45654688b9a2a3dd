#!/usr/bin/env python3
"""GraphMixer inference step on a Wikipedia-shaped synthetic bipartite graph (8,227 + 1,000 nodes, 157,474 edges, seeded 0.5 N(0,1) node
features): B = 200 positive edges per step, K = 30 tokens, time_gap = 2000, 2 Mixer blocks, roots [src ; dst ; neg_dst] = 600 per step, steps
taken from the last `--span` interactions (long histories).  In ONE process, clocks primed as bench.py's legs do:

  hip       dyglib_amd.GraphMixer.compute_step_embeddings, one step per call and `--fuse` steps per call (median of the timed calls, HIP events)
  torch     the SAME model in plain PyTorch-ROCm ops on the same GPU: tests/graphmixer_oracle.py's link_encoder / node_term_dense / output on
            cuda tensors, fed the [n, K] and [n, time_gap] neighbour arrays by this package's own device sampler (so it is not charged for a host
            sampler): what a user has without the HIP path.  The fused size runs in chunks of `--torch-chunk` steps ([n, time_gap, 172] floats
            are 0.83 GB per step)

and the largest |hip - torch| over the compared roots.  With `--plain` only the HIP calls run (profiling under rocprofv3 --kernel-trace --stats).
Also printed: per-step algorithmic counts (node-encoder gather bytes = sum over roots of m * Fn * 4, executed channel-FFN flops).  One JSON line.

    python tools/bench_graphmixer.py [--calls 30 --warmup 5 --fuse 32 | --plain]
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

B, K, G, LAYERS, FN, FT = 200, 30, 2000, 2, 172, 100


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30, help="timed calls per leg (>= 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fuse", type=int, default=32, help="steps per call of the fused leg")
    ap.add_argument("--span", type=int, default=60000, help="steps are drawn from the last SPAN interactions")
    ap.add_argument("--torch-chunk", type=int, default=4, help="steps per chunk of the plain-PyTorch fused leg")
    ap.add_argument("--plain", action="store_true", help="HIP calls only (profiling)")
    a = ap.parse_args()
    from dyglib_amd import GraphMixer, get_neighbor_sampler
    dev = "cuda:0"
    data, nf, ef = syn.make_bipartite_graph(8227, 1000, 157474, seed=0)
    nf[1:] = 0.5 * np.random.RandomState(7).standard_normal(nf[1:].shape).astype(np.float32)
    params = syn.make_graphmixer_params(0, K, num_layers=LAYERS)
    sampler = get_neighbor_sampler(data, "recent", seed=1, device=dev)
    model = GraphMixer(nf, ef, sampler, FT, num_tokens=K, num_layers=LAYERS, dropout=0.1, device=dev)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    model = model.to(dev).eval()
    E = data.num_interactions
    rs, ud = np.random.RandomState(2), np.unique(data.dst_node_ids)
    n_calls = a.calls + a.warmup
    first = E - a.span

    def steps(i0, count):
        """`count` consecutive 200-edge steps from interaction i0 as device tensors (src, dst, neg_dst, t)"""
        sl = slice(i0, i0 + count * B)
        host = (data.src_node_ids[sl], data.dst_node_ids[sl], syn.random_negative_dst(rs, ud, count * B), data.node_interact_times[sl])
        return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in host)
    one = [steps(first + i * B, 1) for i in range(n_calls)]
    n_fused = max(1, (a.span // (a.fuse * B)))
    fused = [steps(first + (i % n_fused) * a.fuse * B, a.fuse) for i in range(n_calls)]

    def hip(s, d, ng, t):
        with torch.no_grad():
            return model.compute_step_embeddings(s, d, ng, t, num_neighbors=K, time_gap=G)

    # ---- the same model in plain PyTorch ops on the GPU -------------------------------------------------------------------------------------
    from tests import graphmixer_oracle as gmo
    P = {k: torch.from_numpy(v).to(dev) for k, v in params.items()}
    nf_d, ef_d = model.node_raw_features, model.edge_raw_features

    def torch_roots(nodes, times):
        nbr, eid, ts = sampler.get_historical_neighbors_device(nodes, times, K)
        dt = (times.unsqueeze(1) - ts.double()).float()
        link = gmo.link_encoder(P, ef_d, nbr, eid, dt, LAYERS)
        gap = sampler.get_historical_neighbors_device(nodes, times, G)[0]
        return gmo.output(P, link, gmo.node_term_dense(nf_d, gap) + nf_d[nodes])

    def plain(s, d, ng, t):
        with torch.no_grad():
            outs = []
            for c0 in range(0, s.numel(), a.torch_chunk * B):
                sl = slice(c0, c0 + a.torch_chunk * B)
                o = torch_roots(torch.cat([s[sl], d[sl], ng[sl]]), torch.cat([t[sl]] * 3))
                outs.append(o.view(3, -1, FN))
            o = torch.cat(outs, dim=1)
            return o[0], o[1], o[2]

    bench._prime_gpu(dev)
    res = {}
    ms_one, out_one = timed(hip, one, a.warmup)
    ms_fused, out_fused = timed(hip, fused, a.warmup)
    res["hip"] = {"one_step_per_call_ms": _stats(ms_one), f"{a.fuse}_steps_per_call_ms": _stats(ms_fused),
                  "edges_per_s_one_step": round(B / (np.median(ms_one) * 1e-3), 1),
                  "edges_per_s_fused": round(a.fuse * B / (np.median(ms_fused) * 1e-3), 1)}
    if not a.plain:
        bench._prime_gpu(dev)
        tms_one, tout_one = timed(plain, one, a.warmup)
        n_t = min(len(fused), 20 + 2)                       # the fused plain leg is long: 20 timed calls after 2
        tms_fused, tout_fused = timed(plain, fused[len(fused) - n_t:], 2)
        res["torch_same_gpu"] = {"one_step_per_call_ms": _stats(tms_one), f"{a.fuse}_steps_per_call_ms": _stats(tms_fused),
                                 "edges_per_s_one_step": round(B / (np.median(tms_one) * 1e-3), 1),
                                 "edges_per_s_fused": round(a.fuse * B / (np.median(tms_fused) * 1e-3), 1),
                                 "what": "tests/graphmixer_oracle.py ops on cuda tensors, neighbour arrays from dygnn_sample_recent; fused leg in chunks of "
                                         f"{a.torch_chunk} steps"}
        res["speedup_vs_torch"] = {"one_step": round(float(np.median(tms_one) / np.median(ms_one)), 2),
                                   "fused": round(float(np.median(tms_fused) / np.median(ms_fused)), 2)}
        res["max_abs_diff_hip_vs_torch"] = max(float((x - y).abs().max()) for x, y in list(zip(out_one, tout_one)) + list(zip(out_fused, tout_fused)))
    # ---- algorithmic counts of the last one-step call ----------------------------------------------------------------------------------------
    s, d, ng, t = one[-1]
    nodes, times = torch.cat([s, d, ng]), torch.cat([t, t, t])
    hist, _ = sampler.hist_len_device(nodes, times)
    m = hist.clamp(max=G).cpu().numpy().astype(np.int64)
    R = 3 * B
    res["per_step"] = {"roots": R, "node_encoder_gather_bytes": int(m.sum()) * FN * 4, "mean_m": round(float(m.mean()), 1), "max_m": int(m.max()),
                       "roots_with_m_0": int((m == 0).sum()),
                       "channel_ffn_flops": R * K * LAYERS * 2 * 2 * FN * 4 * FN, "projection_flops": R * K * 2 * (FN + FT) * FN,
                       "token_ffn_flops": R * LAYERS * FN * 2 * 2 * K * (K // 2), "output_flops": R * 2 * 2 * FN * FN}
    res.update(metric="positive edges/s, GraphMixer inference step (Wikipedia-shaped synthetic graph)", unit="edges/s",
               value=res["hip"]["edges_per_s_fused"],
               config={"batch": B, "num_neighbors": K, "time_gap": G, "num_layers": LAYERS, "roots_per_step": "[src ; dst ; neg_dst]",
                       "timer": "HIP events per call, median", "warmup_calls": a.warmup, "primed": "0.4 s of unrelated matmuls before each leg"})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
