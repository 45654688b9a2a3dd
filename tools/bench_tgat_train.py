#!/usr/bin/env python3
"""Training-step throughput of the TGAT path (BASELINE config 3 trained like train_link_prediction.py:170-185, :242-257): on bench.bench_tgat's
Reddit-shaped graph (10,000 + 984 nodes, 672,447 edges), batch 200, k = 20, 2 layers, `recent` sampling, dropout 0.1, one step = the positive
and the negative compute_src_dst_node_temporal_embeddings call, MergeLayer logits + sigmoid, BCE, backward, torch.optim.Adam.  Beside it a
same-run CPU baseline: the same step through torch autograd on the CPU oracle (oracle/tgat_oracle.py: node_embeddings, the reference's
recursion) on 16 threads, timed like bench._timed_cpu.  One JSON line.

    python tools/bench_tgat_train.py [--steps 20 --warmup 5 --cpu-seconds 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                                    # noqa: E402
from dyglib_amd import synthetic as syn                         # noqa: E402

B, K, FN, FT, DQ, DKV, H = 200, 20, 172, 100, 272, 444, 2
HD = DQ // H
# Executed flops per (node, time) entry.  Forward (bench.py, bench_tgat: 1.062 MFLOP): q 2*272^2, W_k^T q 2*2*136*444, W_v z 2*2*444*136,
# residual_fc 2*272^2, merge fc1 2*444*172, fc2 2*172^2, scores + weighted sums 2*2*20*444*2.  Backward: every product twice (data and
# weight gradient; fc1's data gradient over its 272 non-raw columns only), the attention three times its forward gather products (dp~ = dz.x,
# d(W_k^T q) = sum ds x, dx = p~ dz + ds W_k^T q).
FWD = 2 * DQ * DQ + 2 * H * HD * DKV + 2 * H * DKV * HD + 2 * DQ * DQ + 2 * (DQ + FN) * FN + 2 * FN * FN + 2 * H * K * DKV * 2
BWD = (2 * (2 * DQ * DQ) + 2 * (2 * H * HD * DKV) + 2 * (2 * H * DKV * HD) + 2 * (2 * DQ * DQ) + (2 * FN * DQ + 2 * (DQ + FN) * FN)
       + 2 * (2 * FN * FN) + 2 * H * K * DKV * 4)
ENTRIES = 2 * 2 * B * (1 + K + 1)            # two calls, [src ; dst] = 2B roots each, every root with its 21 level-1 entries: no de-duplication


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-seconds", type=float, default=20.0)
    ap.add_argument("--cpu-max-steps", type=int, default=3)
    a = ap.parse_args()
    from dyglib_amd import TGAT, MergeLayer, get_neighbor_sampler
    from oracle import dygformer_oracle as orc
    from oracle import tgat_oracle as torc
    dev = "cuda:0"
    data, nf, ef = syn.make_bipartite_graph(10000, 984, 672447, seed=0)
    params, mparams = syn.make_tgat_params(0), syn.make_merge_layer_params(1000)
    sampler = get_neighbor_sampler(data, "recent", seed=1, device=dev)
    model = TGAT(nf, ef, sampler, FT, num_layers=2, num_heads=H, dropout=0.1, device=dev)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    merge = MergeLayer(FN, FN, FN, 1)
    merge.load_state_dict({k: torch.from_numpy(v) for k, v in mparams.items()})
    model, merge = model.to(dev).train(), merge.to(dev).train()
    opt = torch.optim.Adam(list(model.parameters()) + list(merge.parameters()), lr=1e-4)
    E = data.num_interactions
    rs, ud = np.random.RandomState(2), np.unique(data.dst_node_ids)
    nb = int(E * 0.7) // B
    host = [(data.src_node_ids[i * B:(i + 1) * B], data.dst_node_ids[i * B:(i + 1) * B], syn.random_negative_dst(rs, ud, B),
             data.node_interact_times[i * B:(i + 1) * B]) for i in range(0, nb, max(1, nb // 64))]
    batches = [tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in h) for h in host]
    bce = torch.nn.functional.binary_cross_entropy

    def step(i):
        s, d, n, t = batches[i % len(batches)]
        ps, pd = model.compute_src_dst_node_temporal_embeddings(s, d, t, num_neighbors=K)
        ns, nd = model.compute_src_dst_node_temporal_embeddings(s, n, t, num_neighbors=K)
        pos, neg = merge(ps, pd).squeeze(-1).sigmoid(), merge(ns, nd).squeeze(-1).sigmoid()
        loss = bce(torch.cat([pos, neg]), torch.cat([torch.ones_like(pos), torch.zeros_like(neg)]))
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss

    torch.manual_seed(0)
    bench._prime_gpu(dev)
    for i in range(a.warmup):
        step(i)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(a.steps):
        last = step(a.warmup + i)
    torch.cuda.synchronize(dev)
    sec = (time.perf_counter() - t0) / a.steps
    loss = float(last.detach())

    # CPU baseline: the same step through torch autograd on the oracle (parameters as leaf tensors, dropout off: eval-mode recursion)
    torch.set_num_threads(bench.cpu_threads())
    adj = orc.OracleAdjacency(data.src_node_ids, data.dst_node_ids, data.edge_ids, data.node_interact_times)
    cp = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in params.items()}
    cmerge = MergeLayer(FN, FN, FN, 1)
    cmerge.load_state_dict({k: torch.from_numpy(v) for k, v in mparams.items()})
    copt = torch.optim.Adam(list(cp.values()) + list(cmerge.parameters()), lr=1e-4)
    nft, eft = torch.from_numpy(nf), torch.from_numpy(ef)

    def cpu_step(i):
        s, d, n, t = host[i % len(host)]
        t = np.asarray(t, dtype=np.float64)
        emb = [torc.node_embeddings(cp, nft, eft, adj, ids, t, 2, K, H) for ids in (s, d, s, n)]
        pos, neg = cmerge(emb[0], emb[1]).squeeze(-1).sigmoid(), cmerge(emb[2], emb[3]).squeeze(-1).sigmoid()
        l = bce(torch.cat([pos, neg]), torch.cat([torch.ones_like(pos), torch.zeros_like(neg)]))
        copt.zero_grad(set_to_none=True)
        l.backward()
        copt.step()
        return float(l.detach())
    n_cpu, cpu_el, _ = bench._timed_cpu(cpu_step, 0, a.cpu_max_steps, a.cpu_seconds)
    cpu_sec = cpu_el / n_cpu
    flop = (FWD + BWD) * ENTRIES
    out = {"metric": "edges/sec (link-prediction training step) TGAT Reddit-shaped (config 3)", "edges_per_s": round(B / sec, 1), "unit": "edges/s",
           "ms_per_step": round(sec * 1e3, 3), "steps": a.steps, "warmup": a.warmup, "final_loss": round(loss, 5),
           "config": {"workload": "TGAT training step: 2 calls (pos, neg) + MergeLayer + BCE + backward + Adam; synthetic Reddit-shaped graph "
                                  "(10000+984 nodes, 672447 edges), k=20, 2 layers, 2 heads, batch=200, recent, dropout 0.1"},
           "roofline": {"bound": "mfma", "achieved": round(flop / sec / 1e12, 3), "peak": bench.PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(flop / sec / (bench.PEAK_F32_MFMA_TFLOPS * 1e12), 4), "flop_per_step": flop,
                        "entries_per_step": ENTRIES, "flop_per_entry": {"forward": FWD, "backward": BWD},
                        "note": "executed flops: every level entry computed (no de-duplication in training), K and V never materialised"},
           "cpu_baseline": {"edges_per_s": round(B / cpu_sec, 2), "ms_per_step": round(cpu_sec * 1e3, 1), "steps": n_cpu, "threads": torch.get_num_threads(),
                            "what": "torch autograd through oracle.tgat_oracle.node_embeddings (the reference recursion), MergeLayer, BCE, Adam"},
           "speedup_vs_cpu": round(cpu_sec / sec, 1)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
