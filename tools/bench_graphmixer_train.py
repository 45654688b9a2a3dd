#!/usr/bin/env python3
"""Training-step time of the GraphMixer path: on a Wikipedia-shaped bipartite graph (seeded 0.5 N(0,1) node features), batch 200, K = 30
tokens, time_gap = 2000, 2 Mixer blocks, `recent` sampling, dropout 0.1, one step = the positive and the negative
compute_src_dst_node_temporal_embeddings call, MergeLayer logits + sigmoid, BCE, backward, torch.optim.Adam on the HIP path
(dygnn_graphmixer_train_forward / dygnn_graphmixer_backward).  Beside it, in the same run on the same GPU, the same model as plain
PyTorch-ROCm autograd: the operations of tests/graphmixer_train_oracle.py on `cuda` (same device sampler for the [n, K] and [n, time_gap]
neighbour arrays, torch-drawn dropout masks).  Clocks primed before each leg, warm-up steps untimed, HIP events around every step, median.
Prints one JSON line and, with --out, writes the two times, their ratio and the executed channel-FFN flops to a text file.

    python tools/bench_graphmixer_train.py [--steps 20 --warmup 5 --out profiles/graphmixer_train_bench.txt] [--hip-only]

--hip-only skips the PyTorch side: the form to put under `rocprofv3 --kernel-trace --stats` for the per-kernel table
(profiles/graphmixer_train_kernel_stats.csv), in a run of its own.
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

B, K, G, L, FN, FT = 200, 30, 2000, 2, 172, 100
PEAK_FP32_MFMA_TFLOPS = 157.3                                   # MI355X, fp32 matrix (the figure DESIGN §4.12 uses)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dyglib_amd import GraphMixer, MergeLayer, get_neighbor_sampler
    from tests import graphmixer_oracle as gmo
    from tests import graphmixer_train_oracle as gto
    dev = "cuda:0"
    data, nf, ef = syn.make_bipartite_graph(8227, 1000, 157474, seed=0)
    nf[1:] = 0.5 * np.random.RandomState(7).standard_normal(nf[1:].shape).astype(np.float32)
    params, mparams = syn.make_graphmixer_params(0, K, num_layers=L), syn.make_merge_layer_params(1000)
    sampler = get_neighbor_sampler(data, "recent", seed=1, device=dev)
    model = GraphMixer(nf, ef, sampler, FT, num_tokens=K, num_layers=L, dropout=0.1, device=dev)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    merge = MergeLayer(FN, FN, FN, 1)
    merge.load_state_dict({k: torch.from_numpy(v) for k, v in mparams.items()})
    model, merge = model.to(dev).train(), merge.to(dev).train()
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad] + list(merge.parameters()), lr=1e-4)
    E = data.num_interactions
    rs, ud = np.random.RandomState(2), np.unique(data.dst_node_ids)
    nb = int(E * 0.7) // B
    host = [(data.src_node_ids[i * B:(i + 1) * B], data.dst_node_ids[i * B:(i + 1) * B], syn.random_negative_dst(rs, ud, B),
             data.node_interact_times[i * B:(i + 1) * B]) for i in range(nb // 2, nb, max(1, nb // 64))]
    batches = [tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in h) for h in host]
    bce = torch.nn.functional.binary_cross_entropy

    def finish(emb, mrg, o):
        ps, pd, ns, nd = emb
        pos, neg = mrg(ps, pd).squeeze(-1).sigmoid(), mrg(ns, nd).squeeze(-1).sigmoid()
        loss = bce(torch.cat([pos, neg]), torch.cat([torch.ones_like(pos), torch.zeros_like(neg)]))
        o.zero_grad(set_to_none=True)
        loss.backward()
        o.step()
        return loss

    kw = dict(num_neighbors=K, time_gap=G)

    def hip_step(i):
        s, d, n, t = batches[i % len(batches)]
        return finish(model.compute_src_dst_node_temporal_embeddings(s, d, t, **kw) + model.compute_src_dst_node_temporal_embeddings(s, n, t, **kw), merge, opt)

    # plain PyTorch: parameters as leaf tensors on the GPU (the time encoder frozen), the restatement's operations, the same sampler
    tp = {k: torch.from_numpy(v.copy()).to(dev).requires_grad_(not k.startswith("time_encoder.")) for k, v in params.items()}
    tmerge = MergeLayer(FN, FN, FN, 1)
    tmerge.load_state_dict({k: torch.from_numpy(v) for k, v in mparams.items()})
    tmerge = tmerge.to(dev).train()
    topt = torch.optim.Adam([p for p in tp.values() if p.requires_grad] + list(tmerge.parameters()), lr=1e-4)
    nft, eft = model.node_raw_features, model.edge_raw_features

    def torch_call(s, d, t):
        nodes, times = torch.cat([s, d]), torch.cat([t, t]).double()
        nbr, eid, ts = sampler.get_historical_neighbors_device(nodes, times, K)
        dt = (times.unsqueeze(1) - ts.double()).float()
        link = gto.link_encoder(tp, eft, nbr, eid, dt, L, 0.1)
        with torch.no_grad():                                    # the node encoder has no parameters
            term = gmo.node_term_dense(nft, sampler.get_historical_neighbors_device(nodes, times, G)[0]) + nft[nodes]
        out = gmo.output(tp, link, term)
        return out[:s.numel()], out[s.numel():]

    def torch_step(i):
        s, d, n, t = batches[i % len(batches)]
        return finish(torch_call(s, d, t) + torch_call(s, n, t), tmerge, topt)

    def timed(step):
        """HIP events around every step (the first `warmup` untimed) -> (median seconds per step, last loss)"""
        marks, last = [], None
        for i in range(a.warmup + a.steps):
            m0, m1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            m0.record()
            last = step(i)
            m1.record()
            if i >= a.warmup:
                marks.append((m0, m1))
        torch.cuda.synchronize(dev)
        return float(np.median([x.elapsed_time(y) for x, y in marks])) * 1e-3, float(last.detach())

    torch.manual_seed(0)
    bench._prime_gpu(dev)
    hip_sec, hip_loss = timed(hip_step)
    # executed flops of the channel FFN products, the bulk of the step: per block and call 2 forward and 4 backward products of 2 R C H flops
    R, C, H = 2 * B * K, FN, 4 * FN
    flops = 2 * L * 6 * 2 * R * C * H
    out = {"metric": "ms per link-prediction training step, GraphMixer", "hip_ms_per_step": round(hip_sec * 1e3, 3), "edges_per_s": round(B / hip_sec, 1),
           "steps": a.steps, "warmup": a.warmup, "final_loss": round(hip_loss, 5), "channel_ffn_gflop_per_step": round(flops * 1e-9, 2),
           "fraction_of_fp32_mfma_peak": round(flops / hip_sec / (PEAK_FP32_MFMA_TFLOPS * 1e12), 4),
           "config": {"workload": "GraphMixer training step: 2 calls (pos, neg) + MergeLayer + BCE + backward + Adam; synthetic Wikipedia-shaped graph "
                                  "(8227+1000 nodes, 157474 edges), K=30, time_gap=2000, 2 blocks, batch=200, recent, dropout 0.1",
                      "timer": "HIP events per step, median", "primed": "before each leg"}}
    if not a.hip_only:
        bench._prime_gpu(dev)
        torch_sec, torch_loss = timed(torch_step)
        out.update({"torch_ms_per_step": round(torch_sec * 1e3, 3), "torch_final_loss": round(torch_loss, 5),
                    "torch_over_hip": round(torch_sec / hip_sec, 3),
                    "torch_what": "torch autograd on the same GPU through tests/graphmixer_train_oracle.py's operations (rocBLAS / eager kernels), same sampler"})
    print(json.dumps(out), flush=True)
    if a.out and not a.hip_only:
        with open(a.out, "w") as f:
            f.write("GraphMixer training step, B = 200, K = 30, time_gap = 2000, 2 blocks, dropout 0.1, one MI355X, median of %d steps after %d warm-up steps\n"
                    % (a.steps, a.warmup))
            f.write("hand-written HIP path : %.3f ms / step\n" % (hip_sec * 1e3))
            f.write("plain PyTorch autograd: %.3f ms / step\n" % (torch_sec * 1e3))
            f.write("PyTorch / HIP         : %.3f\n" % (torch_sec / hip_sec))
            f.write("channel FFN products  : %.2f GFLOP / step executed = %.1f %% of the fp32 MFMA peak (%.1f TFLOP/s) at the HIP time\n"
                    % (flops * 1e-9, 100 * flops / hip_sec / (PEAK_FP32_MFMA_TFLOPS * 1e12), PEAK_FP32_MFMA_TFLOPS))


if __name__ == "__main__":
    main()
