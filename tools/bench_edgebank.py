#!/usr/bin/env python3
"""EdgeBank evaluation on a Wikipedia-shaped synthetic bipartite graph (8,227 + 1,000 nodes, 157,474 chronological edges), split 70 / 15 / 15
by position, test batches of 200 (119 batches, the last one ragged), negatives from a seeded NegativeEdgeSampler, every mode combination.
In ONE process, per mode:

  hip      dyglib_amd.evaluate_edge_bank_link_prediction, whole evaluation per call (table build, every batch's insert + query, metrics kernels,
           one synchronisation): wall time (time.perf_counter around the call, which ends synchronised), median of `--calls` after `--warmup`.
           The host-side np.quantile calls of fixed_proportion are inside that time and are also timed on their own (the same calls, replayed).
           Also the device-only time of the scoring half (table.evaluate over device-resident inputs, HIP events).
  oracle   tests/edgebank_oracle.py doing the reference's per-batch rebuild (a dict / set over train ++ val ++ test prefix per batch) over the
           first `--oracle-batches` batches (the full run is minutes of pure Python; the per-batch time is what is compared), timed once.

Parity between the two is exact (every score of the compared batches) or the tool exits non-zero.  One JSON line.

    python tools/bench_edgebank.py [--calls 10 --warmup 2 --oracle-batches 24]
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
from dyglib_amd.data_loader import Data                         # noqa: E402

B = 200
MODES = [("unlimited_memory", "fixed_proportion"), ("repeat_threshold_memory", "fixed_proportion"),
         ("time_window_memory", "fixed_proportion"), ("time_window_memory", "repeat_interval")]


def _stats(ms):
    ms = np.asarray(ms, dtype=np.float64)
    return {"median": round(float(np.median(ms)), 4), "min": round(float(ms.min()), 4), "max": round(float(ms.max()), 4), "calls": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--oracle-batches", type=int, default=24)
    a = ap.parse_args()
    from dyglib_amd import NegativeEdgeSampler, edgebank as eb, get_idx_data_loader
    from tests import edgebank_oracle as eo
    d, _, _ = syn.make_bipartite_graph(8227, 1000, 157474, seed=0, edge_feat_dim=1, edge_feat_kind="zeros")
    E = d.num_interactions
    n_train, n_hist = int(0.70 * E), int(0.85 * E)
    sub = lambda lo, hi: Data(d.src_node_ids[lo:hi], d.dst_node_ids[lo:hi], d.node_interact_times[lo:hi], d.edge_ids[lo:hi], d.labels[lo:hi])
    train, val, test = sub(0, n_train), sub(n_train, n_hist), sub(n_hist, E)
    n_test = E - n_hist
    batches = [np.arange(lo, min(lo + B, n_test)) for lo in range(0, n_test, B)]
    sampler = NegativeEdgeSampler(d.src_node_ids, d.dst_node_ids, seed=2)
    loader = get_idx_data_loader(list(range(n_test)), batch_size=B, shuffle=False)
    sampler.reset_random_state()
    negs = [(test.src_node_ids[i], sampler.sample(size=len(i))[1]) for i in batches]
    src, dst, t = d.src_node_ids, d.dst_node_ids, d.node_interact_times
    hist = np.array([n_hist + int(i[0]) for i in batches])
    res = {"graph": {"edges": E, "history_before_test": n_hist, "test_edges": n_test, "batch": B, "batches": len(batches)}, "modes": {}}

    for mode, window_mode in MODES:
        key = mode if mode != "time_window_memory" else f"{mode}/{window_mode}"
        run = lambda: eb.evaluate_edge_bank_link_prediction(train, val, loader, sampler, test, edge_bank_memory_mode=mode,
                                                            time_window_mode=window_mode, test_ratio=0.15)
        bench._prime_gpu("cuda:0")
        walls = []
        for i in range(a.calls + a.warmup):
            t0 = time.perf_counter()
            losses, metrics = run()
            if i >= a.warmup:
                walls.append((time.perf_counter() - t0) * 1e3)
        m, wm = eb._modes(mode, window_mode)
        quantile_ms = 0.0
        if (m, wm) == (2, 0):
            t0 = time.perf_counter()
            starts_host = [eb.window_start_time(t[:h], 0.15) for h in hist]
            quantile_ms = (time.perf_counter() - t0) * 1e3
        # device-only: the scoring half over device-resident inputs (full batches in one call, the ragged one in a second)
        full = len(batches) - (1 if len(batches[-1]) < B else 0)
        groups = [(0, full)] + ([(full, len(batches))] if full < len(batches) else [])
        dev_in = []
        for lo, hi in groups:
            qs = torch.from_numpy(np.stack([np.concatenate([src[n_hist + i], n[0]]) for i, n in zip(batches[lo:hi], negs[lo:hi])])).cuda()
            qd = torch.from_numpy(np.stack([np.concatenate([dst[n_hist + i], n[1]]) for i, n in zip(batches[lo:hi], negs[lo:hi])])).cuda()
            st = torch.tensor(starts_host[lo:hi], dtype=torch.float64).cuda() if (m, wm) == (2, 0) else None
            dev_in.append((hist[lo:hi], st, qs, qd))
        table = eb.EdgeBankTable(src, dst, t)
        dev_ms, scores = [], None
        for i in range(a.calls + a.warmup):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            table.reset()
            scores = [table.evaluate(h, st, qs, qd, m, wm) for h, st, qs, qd in dev_in]
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                dev_ms.append(e0.elapsed_time(e1))
        assert int(table.flags().item()) == 0
        got = [row.cpu().numpy().astype(np.float64) for s in scores for row in s]
        # the reference's per-batch rebuild, restated (tests/edgebank_oracle.py), over the first batches
        k = min(a.oracle_batches, len(batches))
        t0 = time.perf_counter()
        want = eo.evaluate(src, dst, t, n_hist, batches, negs, mode, window_mode, 0.15, limit=k)
        oracle_ms = (time.perf_counter() - t0) * 1e3
        mismatches = int(sum((g != w).sum() for g, w in zip(got[:k], want)))
        wall = float(np.median(walls))
        res["modes"][key] = {
            "hip_evaluation_wall_ms": _stats(walls), "hip_per_batch_ms": round(wall / len(batches), 4),
            "of_which_host_np_quantile_ms": round(quantile_ms, 3),
            "hip_device_scoring_ms": _stats(dev_ms), "hip_device_scoring_per_batch_us": round(float(np.median(dev_ms)) * 1e3 / len(batches), 2),
            "oracle_batches": k, "oracle_ms": round(oracle_ms, 1), "oracle_per_batch_ms": round(oracle_ms / k, 2),
            "speedup_per_batch_wall": round((oracle_ms / k) / (wall / len(batches)), 1),
            "score_mismatches_in_compared_batches": mismatches, "scores_compared": int(sum(len(w) for w in want)),
            "mean_loss": round(float(np.mean(losses)), 4), "mean_ap": round(float(np.mean([x["average_precision"] for x in metrics])), 4),
            "mean_auc": round(float(np.mean([x["roc_auc"] for x in metrics])), 4)}
        if mismatches:
            print(json.dumps(res), flush=True)
            sys.exit(f"{key}: {mismatches} scores differ from the oracle")
    cap = eb.table_capacity(E)
    res.update(metric="EdgeBank evaluation wall time per batch (Wikipedia-shaped synthetic graph), unlimited_memory", unit="ms/batch",
               value=res["modes"]["unlimited_memory"]["hip_per_batch_ms"],
               config={"table_slots": cap, "table_bytes": 64 + 2048 + 28 * cap, "timer": "perf_counter around the call (wall), HIP events (device)",
                       "warmup_calls": a.warmup, "primed": "0.4 s of unrelated matmuls before each mode",
                       "oracle": f"tests/edgebank_oracle.py, first {a.oracle_batches} batches, same process, timed once"})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
