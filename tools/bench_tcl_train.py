#!/usr/bin/env python3
"""Training-step time of the TCL path: on a Wikipedia-shaped bipartite graph, batch 200, K = 20, 2 layers, 2 heads, `recent` sampling, dropout
0.1, one step = the positive and the negative compute_src_dst_node_temporal_embeddings call, MergeLayer logits + sigmoid, BCE, backward,
torch.optim.Adam on the HIP path (dygnn_tcl_train_forward / dygnn_tcl_backward).  Beside it, in the same run on the same GPU, the same model
as plain PyTorch-ROCm autograd: the operations of tests/tcl_train_oracle.py on `cuda` (same device sampler, torch-drawn dropout masks).
Prints one JSON line and, with --out, writes the two times and their ratio to a text file.

    python tools/bench_tcl_train.py [--steps 20 --warmup 5 --out profiles/tcl_train_bench.txt] [--hip-only]

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

B, K, L, H, FN, FT = 200, 20, 2, 2, 172, 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dyglib_amd import TCL, MergeLayer, get_neighbor_sampler
    from tests import tcl_oracle as tco
    from tests import tcl_train_oracle as tto
    dev = "cuda:0"
    data, nf, ef = syn.make_bipartite_graph(8227, 1000, 157474, seed=0)
    params, mparams = syn.make_tcl_params(0, K, num_layers=L), syn.make_merge_layer_params(1000)
    sampler = get_neighbor_sampler(data, "recent", seed=1, device=dev)
    model = TCL(nf, ef, sampler, FT, num_layers=L, num_heads=H, num_depths=K + 1, dropout=0.1, device=dev)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    merge = MergeLayer(FN, FN, FN, 1)
    merge.load_state_dict({k: torch.from_numpy(v) for k, v in mparams.items()})
    model, merge = model.to(dev).train(), merge.to(dev).train()
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
        sides = [tco.encoder_input(tp, nft, eft, ids, t, *sampler.get_historical_neighbors_device(ids, t, K)) for ids in (s, d)]
        return tto.layers(tp, sides[0][0], sides[0][1], sides[1][0], sides[1][1], L, H, 0.1)

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
    out = {"metric": "ms per link-prediction training step, TCL", "hip_ms_per_step": round(hip_sec * 1e3, 3), "edges_per_s": round(B / hip_sec, 1),
           "steps": a.steps, "warmup": a.warmup, "final_loss": round(hip_loss, 5),
           "config": {"workload": "TCL training step: 2 calls (pos, neg) + MergeLayer + BCE + backward + Adam; synthetic Wikipedia-shaped graph "
                                  "(8227+1000 nodes, 157474 edges), K=20, 2 layers, 2 heads, batch=200, recent, dropout 0.1"}}
    if not a.hip_only:
        torch_sec, torch_loss = timed(torch_step)
        out.update({"torch_ms_per_step": round(torch_sec * 1e3, 3), "torch_final_loss": round(torch_loss, 5),
                    "torch_over_hip": round(torch_sec / hip_sec, 3),
                    "torch_what": "torch autograd on the same GPU through tests/tcl_train_oracle.py's operations (rocBLAS / eager kernels), same sampler"})
    print(json.dumps(out), flush=True)
    if a.out and not a.hip_only:
        with open(a.out, "w") as f:
            f.write("TCL training step, B = 200, K = 20, 2 layers, 2 heads, dropout 0.1, one MI355X, %d steps after %d warm-up steps\n" % (a.steps, a.warmup))
            f.write("hand-written HIP path : %.3f ms / step\n" % (hip_sec * 1e3))
            f.write("plain PyTorch autograd: %.3f ms / step\n" % (torch_sec * 1e3))
            f.write("PyTorch / HIP         : %.3f\n" % (torch_sec / hip_sec))


if __name__ == "__main__":
    main()
