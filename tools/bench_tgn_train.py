#!/usr/bin/env python3
"""Training-step time of the TGN path (BASELINE config 5 trained like train_link_prediction.py:186-207, :242-264): on bench.bench_tgn's
MOOC-shaped graph (7,047 + 97 nodes, 411,749 edges), batch 200, k = 10, 1 layer, `recent` sampling, dropout 0.1, batches in chronological order
from interaction 0; one step = the negative and the positive compute_src_dst_node_temporal_embeddings call (the positive one updates the
memory bank), MergeLayer logits + sigmoid, BCE, backward, torch.optim.Adam, detach_memory_bank.  Every step is timed with HIP events (whole
step, and its forward / backward / optimiser parts); reported: the median over the timed steps and their spread.  Beside it, from the same
run: the inference step of the same model on the same batches (two calls, no_grad, as tools/bench_tgn.py --two-calls), and a CPU baseline,
the same training step through torch autograd on the test-side composition of the CPU oracle (tests/tgn_autograd.py).  One JSON line.

    python tools/bench_tgn_train.py [--steps 40 --warmup 20 --cpu-seconds 20 | --no-cpu]
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

B, K, FN = 200, 10, 172


def _stats(ms):
    ms = np.asarray(ms, dtype=np.float64)
    return {"median": round(float(np.median(ms)), 4), "min": round(float(ms.min()), 4), "p90": round(float(np.percentile(ms, 90)), 4),
            "max": round(float(ms.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cpu-seconds", type=float, default=20.0)
    ap.add_argument("--cpu-max-steps", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU baseline (profiling runs)")
    a = ap.parse_args()
    from dyglib_amd import MemoryModel, MergeLayer, get_neighbor_sampler
    dev = "cuda:0"
    data, nf, ef = syn.make_bipartite_graph(7047, 97, 411749, seed=0, edge_feat_kind="sparse4")
    params, mparams = syn.make_tgn_params(0, nf.shape[0], num_layers=1), syn.make_merge_layer_params(1000)
    sampler = get_neighbor_sampler(data, "recent", seed=1, device=dev)
    model = MemoryModel(nf, ef, sampler, 100, model_name="TGN", num_layers=1, num_heads=2, dropout=0.1, device=dev)
    sd = model.state_dict()
    sd.update({k: torch.from_numpy(v) for k, v in params.items()})
    model.load_state_dict(sd)
    merge = MergeLayer(FN, FN, FN, 1)
    merge.load_state_dict({k: torch.from_numpy(v) for k, v in mparams.items()})
    model, merge = model.to(dev), merge.to(dev)
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad] + list(merge.parameters()), lr=1e-4)
    rs, ud = np.random.RandomState(2), np.unique(data.dst_node_ids)
    n = a.steps + a.warmup
    host = [(data.src_node_ids[i * B:(i + 1) * B], data.dst_node_ids[i * B:(i + 1) * B], syn.random_negative_dst(rs, ud, B),
             data.node_interact_times[i * B:(i + 1) * B], data.edge_ids[i * B:(i + 1) * B]) for i in range(n)]
    batches = [tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in b) for b in host]
    bce = torch.nn.functional.binary_cross_entropy
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def calls(i):
        s, d, ng, t, e = batches[i]
        ns, nd = model.compute_src_dst_node_temporal_embeddings(s, ng, t, edge_ids=None, edges_are_positive=False, num_neighbors=K)
        ps, pd = model.compute_src_dst_node_temporal_embeddings(s, d, t, edge_ids=e, edges_are_positive=True, num_neighbors=K)
        return ns, nd, ps, pd

    def train_step(i):
        marks = [ev() for _ in range(4)]
        marks[0].record()
        ns, nd, ps, pd = calls(i)
        pos, neg = merge(ps, pd).squeeze(-1).sigmoid(), merge(ns, nd).squeeze(-1).sigmoid()
        loss = bce(torch.cat([pos, neg]), torch.cat([torch.ones_like(pos), torch.zeros_like(neg)]))
        marks[1].record()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        marks[2].record()
        opt.step()
        model.memory_bank.detach_memory_bank()
        marks[3].record()
        return loss, marks

    def infer_step(i):
        m0, m1 = ev(), ev()
        m0.record()
        with torch.no_grad():
            ns, nd, ps, pd = calls(i)
            merge.link_probabilities(ps, pd), merge.link_probabilities(ns, nd)
        m1.record()
        return m0, m1

    def run(step, mode):
        model.train(mode), merge.train(mode)
        model.memory_bank.__init_memory_bank__()
        bench._prime_gpu(dev)
        out = [step(i) for i in range(n)]
        torch.cuda.synchronize(dev)
        return out[a.warmup:]
    torch.manual_seed(0)
    inf = [m0.elapsed_time(m1) for m0, m1 in run(infer_step, False)]
    timed = run(train_step, True)
    loss = float(timed[-1][0].detach())
    total = [m[0].elapsed_time(m[3]) for _, m in timed]
    parts = {name: _stats([m[j].elapsed_time(m[j + 1]) for _, m in timed]) for j, name in enumerate(("forward", "backward", "optimizer"))}
    ms = float(np.median(total))

    # CPU baseline: the same step through torch autograd on the oracle composition (parameters as leaf tensors, dropout off), the memory bank
    # carried through the same chronological batches
    from oracle import tgn_oracle as norc
    from tests import tgn_autograd as ta
    torch.set_num_threads(bench.cpu_threads())
    adj = ta.adjacency(data)
    cp = ta.grad_params(params)
    st = norc.TgnState(nf.shape[0], FN)
    cmerge = MergeLayer(FN, FN, FN, 1)
    cmerge.load_state_dict({k: torch.from_numpy(v) for k, v in mparams.items()})
    copt = torch.optim.Adam([p for p in cp.values() if p.requires_grad] + list(cmerge.parameters()), lr=1e-4)

    def cpu_step(i):
        s, d, ng, t, e = host[i]
        ns, nd = ta.tgn_call(cp, nf, ef, adj, st, s, ng, t, None, False, 1, K)
        ps, pd = ta.tgn_call(cp, nf, ef, adj, st, s, d, t, e, True, 1, K)
        pos, neg = cmerge(ps, pd).squeeze(-1).sigmoid(), cmerge(ns, nd).squeeze(-1).sigmoid()
        l = bce(torch.cat([pos, neg]), torch.cat([torch.ones_like(pos), torch.zeros_like(neg)]))
        copt.zero_grad(set_to_none=True)
        l.backward()
        copt.step()
        return float(l.detach())
    n_cpu, cpu_el = 0, float("nan")
    if not a.no_cpu:
        n_cpu, cpu_el, _ = bench._timed_cpu(cpu_step, 0, a.cpu_max_steps, a.cpu_seconds)
    cpu_sec = cpu_el / max(n_cpu, 1)
    out = {"metric": "ms per link-prediction training step, TGN MOOC-shaped (config 5)", "ms_per_step": _stats(total), "unit": "ms",
           "edges_per_s": round(B / (ms * 1e-3), 1), "steps": a.steps, "warmup": a.warmup, "final_loss": round(loss, 5), "timer": "HIP events per step",
           "split_ms": parts,
           "config": {"workload": "TGN training step: negative call + positive call (memory update) + MergeLayer + BCE + backward + Adam + "
                                  "detach_memory_bank; synthetic MOOC-shaped graph (7047+97 nodes, 411749 edges), k=10, 1 layer, 2 heads, batch=200, "
                                  "recent, dropout 0.1, sequential batches from interaction 0"},
           "inference_step_ms": dict(_stats(inf), what="the same two calls + MergeLayer + sigmoid under no_grad in eval mode, same batches"),
           "cpu_baseline": {"ms_per_step": round(cpu_sec * 1e3, 1) if n_cpu else None, "steps": n_cpu, "threads": torch.get_num_threads(),
                            "what": "torch autograd through tests/tgn_autograd.py (the CPU oracle's GRU update and recursion), MergeLayer, BCE, Adam; "
                                    "includes the oracle's second, no_grad pass for the state commit"},
           "speedup_vs_cpu": round(cpu_sec * 1e3 / ms, 1) if n_cpu else None}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
