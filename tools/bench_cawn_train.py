#!/usr/bin/env python3
"""Training-step time of the CAWN path: on a Wikipedia-shaped bipartite graph, batch 200, the reference's Wikipedia configuration (one hop,
32 neighbours, position_feat_dim 172, 8 heads: attention_dim 312), `recent` sampling, dropout 0.1, one step = the positive and the negative
compute_src_dst_node_temporal_embeddings call, MergeLayer logits + sigmoid, BCE, backward, torch.optim.Adam on the HIP path
(dygnn_cawn_train_forward / dygnn_cawn_backward after enable_training()).  Beside it, in the same run on the same GPU, the same model as plain
PyTorch-ROCm autograd: the operations of tests/cawn_train_oracle.py on `cuda` (same device sampler, torch-drawn dropout masks).  Prints one
JSON line (with the executed GFLOP per step of the HIP path's products) and, with --out, writes the two times and their ratio to a text file.

    python tools/bench_cawn_train.py [--steps 20 --warmup 5 --out profiles/cawn_train_bench.txt] [--hip-only]

--hip-only skips the PyTorch side: the form to put under `rocprofv3 --kernel-trace --stats` for the per-kernel table.
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

B, K, W, P, HEADS, FN, FE, FT = 200, 32, 1, 172, 8, 172, 172, 100
PEAK_FP32_MFMA_TFLOPS = 157.3                                   # MI355X, v_mfma_f32_*_f32


def step_gflop():
    """multiply-adds x 2 of the products one training step (two calls) executes on the HIP path, as cawn_train.hip lays them out"""
    D = FN + FE + FT + P
    A = syn.cawn_attention_dim(D, HEADS)
    M, T = K ** W, 1 + K + (K * K if W == 2 else 0)
    I = 2 * B
    NT, R, PR, E = I * T, I * M, B * 2 * T, D + P
    parents = [I * K ** lv for lv in range(W)]
    f = 2 * PR * P * P                                                        # position MLP, second layer
    for H, n_in in ((D // 2, D), (P // 2, P)):
        f += 2 * 2 * NT * 4 * H * n_in + sum(2 * n * 4 * H * H for n in parents)      # W_ih both directions, W_hh on the parents
    block = 2 * R * E * A + 2 * R * A * 3 * A + 4 * R * M * A + 2 * R * A * A + 2 * 2 * R * A * 4 * A
    f += block + 2 * I * A * FN
    b = 2 * (block + 2 * I * A * FN) + 4 * R * M * A                          # dX and dW of every product; the attention backward has four
    for H, n_in, dx in ((D // 2, D, FT + P), (P // 2, P, P)):
        b += 2 * (2 * NT * 4 * H * n_in + 2 * NT * 4 * H * dx) + sum(2 * 2 * n * 4 * H * H for n in parents)
    b += 2 * 2 * PR * P * P
    return 2 * (f + b) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dyglib_amd import CAWN, MergeLayer, get_neighbor_sampler
    from tests import cawn_train_oracle as cto
    dev = "cuda:0"
    data, nf, ef = syn.make_bipartite_graph(8227, 1000, 157474, seed=0)
    params, mparams = syn.make_cawn_params(0, P, W, HEADS), syn.make_merge_layer_params(1000)
    sampler = get_neighbor_sampler(data, "recent", seed=1, device=dev)
    model = CAWN(nf, ef, sampler, FT, P, walk_length=W, num_walk_heads=HEADS, dropout=0.1, device=dev)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    merge = MergeLayer(FN, FN, FN, 1)
    merge.load_state_dict({k: torch.from_numpy(v) for k, v in mparams.items()})
    model, merge = model.to(dev).train().enable_training(), merge.to(dev).train()
    opt = torch.optim.Adam(list(model.parameters()) + list(merge.parameters()), lr=1e-4)
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

    def hip_step(i):
        s, d, n, t = batches[i % len(batches)]
        return finish(model.compute_src_dst_node_temporal_embeddings(s, d, t, num_neighbors=K)
                      + model.compute_src_dst_node_temporal_embeddings(s, n, t, num_neighbors=K), merge, opt)

    # plain PyTorch: parameters as leaf tensors on the GPU, the restatement's operations, the same sampler calls in the same order
    tp = {k: torch.from_numpy(v.copy()).to(dev).requires_grad_(True) for k, v in params.items()}
    tmerge = MergeLayer(FN, FN, FN, 1)
    tmerge.load_state_dict({k: torch.from_numpy(v) for k, v in mparams.items()})
    tmerge = tmerge.to(dev).train()
    topt = torch.optim.Adam(list(tp.values()) + list(tmerge.parameters()), lr=1e-4)
    nft, eft = model.node_raw_features, model.edge_raw_features

    def torch_call(s, d, t):
        t = t.double()
        n = s.numel()
        _, _, hops = model._sample([s, d], t, K)
        halves = [[tuple(x[sl] for x in h) for h in hops] for sl in (slice(0, n), slice(n, 2 * n))]
        return cto.forward(tp, nft, eft, s, d, t, halves[0], halves[1], HEADS, 0.1)

    def torch_step(i):
        s, d, n, t = batches[i % len(batches)]
        return finish(torch_call(s, d, t) + torch_call(s, n, t), tmerge, topt)

    def timed(step):
        for i in range(a.warmup):
            step(i)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i in range(a.steps):
            last = step(a.warmup + i)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / a.steps, float(last.detach())

    torch.manual_seed(0)
    bench._prime_gpu(dev)
    hip_sec, hip_loss = timed(hip_step)
    gflop = step_gflop()
    out = {"metric": "ms per link-prediction training step, CAWN", "hip_ms_per_step": round(hip_sec * 1e3, 3), "edges_per_s": round(B / hip_sec, 1),
           "steps": a.steps, "warmup": a.warmup, "final_loss": round(hip_loss, 5), "gflop_per_step": round(gflop, 2),
           "fraction_of_fp32_mfma_peak": round(gflop / hip_sec / 1e3 / PEAK_FP32_MFMA_TFLOPS, 4),
           "config": {"workload": "CAWN training step: 2 calls (pos, neg) + MergeLayer + BCE + backward + Adam; synthetic Wikipedia-shaped graph "
                                  "(8227+1000 nodes, 157474 edges), walk_length 1, 32 neighbours, position_feat_dim 172, 8 heads, batch=200, recent, "
                                  "dropout 0.1"}}
    if not a.hip_only:
        torch_sec, torch_loss = timed(torch_step)
        out.update({"torch_ms_per_step": round(torch_sec * 1e3, 3), "torch_final_loss": round(torch_loss, 5),
                    "torch_over_hip": round(torch_sec / hip_sec, 3),
                    "torch_what": "torch autograd on the same GPU through tests/cawn_train_oracle.py's operations (rocBLAS / eager kernels), same sampler"})
    print(json.dumps(out), flush=True)
    if a.out and not a.hip_only:
        with open(a.out, "w") as f:
            f.write("CAWN training step, B = 200, walk_length 1, 32 neighbours, position_feat_dim 172, 8 heads, dropout 0.1, one MI355X, "
                    "%d steps after %d warm-up steps\n" % (a.steps, a.warmup))
            f.write("hand-written HIP path : %.3f ms / step (%.1f GFLOP / step executed, %.1f %% of the fp32-MFMA peak)\n"
                    % (hip_sec * 1e3, gflop, 100 * gflop / hip_sec / 1e3 / PEAK_FP32_MFMA_TFLOPS))
            f.write("plain PyTorch autograd: %.3f ms / step\n" % (torch_sec * 1e3))
            f.write("PyTorch / HIP         : %.3f\n" % (torch_sec / hip_sec))


if __name__ == "__main__":
    main()
