#!/usr/bin/env python3
"""JODIE and DyRep at TGN's benchmark shape (tools/bench_tgn.py: MOOC-shaped synthetic graph, batch 200, batches strictly in chronological order from
interaction 0, negative call + positive call per step): the HIP path (dygnn_jodie_forward_step, one library call per step) against the same
model written in plain PyTorch-ROCm ops, on the same GPU in the same run, each on a memory bank of its own, with parity between the two on
every timed step and on the banks they leave.  Both are timed over alternating windows, for JODIE (TorchJodie) and for DyRep (TorchDyRep, k = 10, 1 layer).  One JSON line per model; --out appends a text report.

    python tools/bench_memory_variants.py [--steps 100] [--warmup 60] [--windows 5] [--out profiles/memory_variants_bench.txt]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_memory_variants.py --hip-only        (per-kernel times, a run of its own)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dyglib_amd import synthetic as syn  # noqa: E402

B = 200


class TorchJodie:
    """MemoryModel('JODIE') (models/MemoryModel.py:87-168) as batched PyTorch ops on the device: the joint step on [positives ; negatives], one
    pending message per node, the last stored message of a node found with a scatter-max over entry indices."""

    def __init__(self, params, edge_feat, num_nodes, shifts, dev):
        self.p = {k: torch.from_numpy(v).to(dev) for k, v in params.items()}
        self.ef = torch.from_numpy(edge_feat).to(dev)
        Fn = params["memory_updater.memory_updater.weight_hh"].shape[0]
        Dm = params["memory_updater.memory_updater.weight_ih"].shape[1]
        self.M, self.U = torch.zeros((num_nodes, Fn), device=dev), torch.zeros(num_nodes, device=dev)
        self.msg, self.msg_t = torch.zeros((num_nodes, Dm), device=dev), torch.zeros(num_nodes, dtype=torch.float64, device=dev)
        self.has = torch.zeros(num_nodes, dtype=torch.bool, device=dev)
        self.mean = torch.tensor([shifts[0], shifts[2]], dtype=torch.float32, device=dev)
        self.std = torch.tensor([shifts[1], shifts[3]], dtype=torch.float32, device=dev)
        self.last = torch.empty(num_nodes, dtype=torch.int64, device=dev)

    @staticmethod
    def lin1(x, w, b):
        """nn.Linear(1, F) as ONE rounding (the float64 product of two float32 is exact): what the reference's host addmm and the library's
        fmaf compute.  Time differences reach 1e6 here, where rounding the product first moves the cosine in its second digit."""
        return (x.double()[:, None] * w.double().reshape(1, -1) + b.double()[None, :]).float()

    def updated(self, nodes):
        """(pending flag, updated memory, last update after the update) of the rows `nodes`: the RNN cell where a message is pending"""
        p, F = self.p, torch.nn.functional
        has, h = self.has[nodes], self.M[nodes]
        c = "memory_updater.memory_updater."
        new = torch.tanh(F.linear(self.msg[nodes], p[c + "weight_ih"], p[c + "bias_ih"]) + F.linear(h, p[c + "weight_hh"], p[c + "bias_hh"]))
        return has, torch.where(has[:, None], new, h), torch.where(has, self.msg_t[nodes].float(), self.U[nodes])

    def commit(self, nodes, n, n_pos, has, upd, lu, t, eid, other=None):
        """the commit of the positive pairs: entry e = role * n_pos + i; the last entry of a node stores its message.  other (DyRep): the rows
        [n_pos sources ; n_pos destinations] whose partner row is the other endpoint's part of a message"""
        p, dev = self.p, nodes.device
        rows = torch.cat([torch.arange(n_pos, device=dev), n + torch.arange(n_pos, device=dev)])
        orow = torch.cat([n + torch.arange(n_pos, device=dev), torch.arange(n_pos, device=dev)])
        ids = nodes[rows]
        e = torch.arange(2 * n_pos, device=dev)
        win = self.last.fill_(-1).scatter_reduce_(0, ids, e, "amax")[ids] == e
        pend = has[rows]
        w = ids[win & pend]
        self.M[w], self.U[w] = upd[rows][win & pend], lu[rows][win & pend]
        tp = t.float()[:n_pos].repeat(2)
        tf = torch.cos(self.lin1(tp - lu[rows], p["time_encoder.w.weight"], p["time_encoder.w.bias"]))
        mo = upd[orow] if other is None else torch.cat([other[n_pos:], other[:n_pos]])
        m = torch.cat([upd[rows], mo, tf, self.ef[eid[:n_pos].repeat(2)]], dim=1)
        w = ids[win]
        self.msg[w], self.msg_t[w], self.has[w] = m[win], t[:n_pos].repeat(2)[win], True

    def step(self, src, dst, t, eid, n_pos):
        p = self.p
        n = src.numel()
        nodes = torch.cat([src, dst])
        has, upd, lu = self.updated(nodes)
        t32 = t.float()
        delta = (torch.cat([t32, t32]) - lu - self.mean.repeat_interleave(n)) / self.std.repeat_interleave(n)
        emb = upd * (1 + self.lin1(delta, p["embedding_module.linear_layer.weight"], p["embedding_module.linear_layer.bias"]))
        self.commit(nodes, n, n_pos, has, upd, lu, t, eid)
        return emb[:n], emb[n:]


class TorchDyRep(TorchJodie):
    """MemoryModel('DyRep') with one attention layer and `recent` sampling as batched PyTorch ops on the device: the rows returned are the updated
    memories of the roots; for the positive pairs the temporal attention of models/modules.py:137-206 and the MergeLayer over updated memory + raw
    features of the roots and their k most recent neighbours (looked up with the library's sampler, on the device), whose rows enter the messages."""

    def __init__(self, params, node_feat, edge_feat, shifts, sampler, k, heads, dev):
        super().__init__(params, edge_feat, node_feat.shape[0], shifts, dev)
        self.nf, self.sampler, self.k, self.heads = torch.from_numpy(node_feat).to(dev), sampler, k, heads

    def step(self, src, dst, t, eid, n_pos):
        p, F, k, H = self.p, torch.nn.functional, self.k, self.heads
        n = src.numel()
        nodes = torch.cat([src, dst])
        has, upd, lu = self.updated(nodes)
        r, tr = torch.cat([src[:n_pos], dst[:n_pos]]), torch.cat([t[:n_pos], t[:n_pos]])
        nbr, ne, nts = self.sampler.get_historical_neighbors_device(r, tr, k)
        ids = torch.cat([r, nbr.reshape(-1)])
        feat = self.updated(ids)[1] + self.nf[ids]                                          # MemoryModel.py:609
        h_self, h_nbr = feat[:2 * n_pos], feat[2 * n_pos:].reshape(2 * n_pos, k, -1)
        tw, tb = p["time_encoder.w.weight"], p["time_encoder.w.bias"]
        t_self = torch.cos(self.lin1(torch.zeros(2 * n_pos, device=r.device), tw, tb))
        t_nbr = torch.cos(self.lin1((tr[:, None] - nts.double()).float().reshape(-1), tw, tb)).reshape(2 * n_pos, k, -1)
        a = "embedding_module.temporal_conv_layers.0."
        q_in = torch.cat([h_self, t_self], dim=1)
        kv_in = torch.cat([h_nbr, self.ef[ne], t_nbr], dim=2)
        Dq = q_in.shape[1]
        hd = Dq // H
        q = F.linear(q_in, p[a + "query_projection.weight"]).reshape(-1, 1, H, hd).permute(0, 2, 1, 3)
        key = F.linear(kv_in, p[a + "key_projection.weight"]).reshape(-1, k, H, hd).permute(0, 2, 1, 3)
        val = F.linear(kv_in, p[a + "value_projection.weight"]).reshape(-1, k, H, hd).permute(0, 2, 1, 3)
        att = (torch.einsum("bhld,bhnd->bhln", q, key) * hd ** -0.5).masked_fill((nbr == 0)[:, None, None, :], -1e10)
        o = torch.einsum("bhln,bhnd->bhld", torch.softmax(att, dim=-1), val).permute(0, 2, 1, 3).reshape(-1, Dq)
        o = F.layer_norm(F.linear(o, p[a + "residual_fc.weight"], p[a + "residual_fc.bias"]) + q_in, (Dq,), p[a + "layer_norm.weight"], p[a + "layer_norm.bias"], 1e-5)
        g = "embedding_module.merge_layers.0."
        emb = F.linear(F.relu(F.linear(torch.cat([o, h_self], dim=1), p[g + "fc1.weight"], p[g + "fc1.bias"])), p[g + "fc2.weight"], p[g + "fc2.bias"])
        self.commit(nodes, n, n_pos, has, upd, lu, t, eid, other=emb)
        return upd[:n], upd[n:]


def bench_dyrep(a, data, nf, ef, dev):
    """DyRep's step (k = 10, 1 layer: TGN's benchmark configuration): the HIP path against TorchDyRep, each on a memory bank of its own, over
    alternating windows, with parity between the two on every step and on the banks they leave"""
    from dyglib_amd import DyRep, get_neighbor_sampler
    K = 10
    params = syn.make_dyrep_params(0, nf.shape[0], num_layers=1)
    sampler = get_neighbor_sampler(data, "recent", seed=1, device=dev)
    model = DyRep(nf, ef, sampler, 100, num_layers=1, num_heads=2, dropout=0.1, device=dev)
    sd = model.state_dict(); sd.update({k: torch.from_numpy(v) for k, v in params.items()}); model.load_state_dict(sd)
    model = model.to(dev).eval()
    model.memory_bank.__init_memory_bank__()
    plain = TorchDyRep(params, nf, ef, (0.0, 1.0, 0.0, 1.0), sampler, K, 2, dev)
    rs, ud = np.random.RandomState(2), np.unique(data.dst_node_ids)
    joint = []
    for i in range(a.warmup + a.steps * a.windows):
        sl = slice(i * B, (i + 1) * B)
        s_, d_, t_, e_ = data.src_node_ids[sl], data.dst_node_ids[sl], data.node_interact_times[sl], data.edge_ids[sl]
        n_ = syn.random_negative_dst(rs, ud, B)
        joint.append(tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (np.concatenate([s_, s_]), np.concatenate([d_, n_]), np.concatenate([t_, t_]), e_)))
    hip = lambda i: model.compute_step_embeddings_joint(*joint[i], B, num_neighbors=K)
    tor = lambda i: plain.step(*joint[i], B)
    err, times = 0.0, {"hip": [], "torch": []}
    with torch.no_grad():
        for i in range(a.warmup):
            x = hip(i)
            if not a.hip_only:
                y = tor(i)
                err = max(err, float((x[0] - y[0]).abs().max()), float((x[1] - y[1]).abs().max()))
        for w in range(a.windows):
            lo = a.warmup + w * a.steps
            for name, fn in (("hip", hip),) if a.hip_only else (("hip", hip), ("torch", tor)):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                outs = [fn(lo + i) for i in range(a.steps)]
                torch.cuda.synchronize(dev)
                times[name].append((time.perf_counter() - t0) / a.steps * 1e3)
                if name == "hip":
                    kept = outs
                else:
                    err = max([err] + [float((x[k] - y[k]).abs().max()) for x, y in zip(kept, outs) for k in (0, 1)])
    out = {"metric": "ms per step (link-prediction fwd, negative + positive call) DyRep MOOC-shaped, batch 200, k=10, 1 layer", "steps": a.steps,
           "warmup": a.warmup, "windows": a.windows, "hip_ms_per_step": [round(x, 4) for x in times["hip"]],
           "hip_ms_per_step_median": round(float(np.median(times["hip"])), 4)}
    if not a.hip_only:
        out.update({"torch_ms_per_step": [round(x, 4) for x in times["torch"]], "torch_ms_per_step_median": round(float(np.median(times["torch"])), 4),
                    "parity_max_abs_rows": err, "parity_max_abs_memory": float((model.memory_bank.node_memories.data - plain.M).abs().max()),
                    "parity_max_abs_messages": float((model.memory_bank.msg - plain.msg).abs().max()),
                    "parity_has_msg_equal": bool(torch.equal(model.memory_bank.has_msg != 0, plain.has))})
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    if not a.hip_only:
        assert out["parity_max_abs_rows"] <= 1e-4 and out["parity_max_abs_memory"] <= 1e-4 and out["parity_max_abs_messages"] <= 1e-4 and out["parity_has_msg_equal"], \
            "the two DyRep paths disagree"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100); ap.add_argument("--warmup", type=int, default=60); ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--hip-only", action="store_true", help="the HIP path alone, for a kernel trace")
    ap.add_argument("--out", default=None)
    ap.add_argument("--model", default="both", choices=["both", "jodie", "dyrep"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_memory_variants: no GPU (there is no CPU fallback and no CPU timing)")
    from dyglib_amd import JODIE, compute_src_dst_node_time_shifts
    dev = "cuda:0"
    data, nf, ef = syn.make_bipartite_graph(7047, 97, 411749, seed=0, edge_feat_kind="sparse4")
    if a.model in ("both", "dyrep"):
        bench_dyrep(a, data, nf, ef, dev)
    if a.model == "dyrep":
        return
    params = syn.make_jodie_params(0)
    n_steps = a.warmup + a.steps * a.windows
    n_train = int(0.7 * data.num_interactions)
    shifts = tuple(float(x) for x in compute_src_dst_node_time_shifts(data.src_node_ids[:n_train], data.dst_node_ids[:n_train], data.node_interact_times[:n_train]))
    model = JODIE(nf, ef, None, 100, src_node_mean_time_shift=shifts[0], src_node_std_time_shift=shifts[1], dst_node_mean_time_shift_dst=shifts[2],
                  dst_node_std_time_shift=shifts[3], device=dev)
    sd = model.state_dict(); sd.update({k: torch.from_numpy(v) for k, v in params.items()}); model.load_state_dict(sd)
    model = model.to(dev).eval()
    model.memory_bank.__init_memory_bank__()
    plain = TorchJodie(params, ef, nf.shape[0], shifts, dev)
    rs, ud = np.random.RandomState(2), np.unique(data.dst_node_ids)
    joint = []
    for i in range(n_steps):
        sl = slice(i * B, (i + 1) * B)
        s_, d_, t_, e_ = data.src_node_ids[sl], data.dst_node_ids[sl], data.node_interact_times[sl], data.edge_ids[sl]
        n_ = syn.random_negative_dst(rs, ud, B)
        joint.append(tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (np.concatenate([s_, s_]), np.concatenate([d_, n_]), np.concatenate([t_, t_]), e_)))

    def hip(i):
        s2, d2, t2, e2 = joint[i]
        return model.compute_step_embeddings_joint(s2, d2, t2, e2, B)

    def tor(i):
        s2, d2, t2, e2 = joint[i]
        return plain.step(s2, d2, t2, e2, B)
    err = 0.0
    times = {"hip": [], "torch": []}
    with torch.no_grad():
        for i in range(a.warmup):
            x = hip(i)
            if not a.hip_only:
                y = tor(i)
                err = max(err, float((x[0] - y[0]).abs().max()), float((x[1] - y[1]).abs().max()))
        torch.cuda.synchronize(dev)
        for w in range(a.windows):
            lo = a.warmup + w * a.steps
            for name, fn in (("hip", hip),) if a.hip_only else (("hip", hip), ("torch", tor)):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                outs = [fn(lo + i) for i in range(a.steps)]
                torch.cuda.synchronize(dev)
                times[name].append((time.perf_counter() - t0) / a.steps * 1e3)
                if name == "hip":
                    kept = outs
                else:
                    err = max([err] + [float((x[k] - y[k]).abs().max()) for x, y in zip(kept, outs) for k in (0, 1)])
    out = {"metric": "ms per step (link-prediction fwd, negative + positive call) JODIE MOOC-shaped, batch 200", "steps": a.steps, "warmup": a.warmup,
           "windows": a.windows, "hip_ms_per_step": [round(x, 4) for x in times["hip"]], "hip_ms_per_step_median": round(float(np.median(times["hip"])), 4)}
    if not a.hip_only:
        bank = float((model.memory_bank.node_memories.data - plain.M).abs().max())
        out.update({"torch_ms_per_step": [round(x, 4) for x in times["torch"]], "torch_ms_per_step_median": round(float(np.median(times["torch"])), 4),
                    "parity_max_abs_rows": err, "parity_max_abs_memory": bank,
                    "parity_has_msg_equal": bool(torch.equal(model.memory_bank.has_msg != 0, plain.has))})
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    if not a.hip_only:
        assert out["parity_max_abs_rows"] <= 1e-4 and out["parity_max_abs_memory"] <= 1e-4 and out["parity_has_msg_equal"], "the two paths disagree"


if __name__ == "__main__":
    main()
