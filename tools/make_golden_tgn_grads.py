#!/usr/bin/env python3
"""Gradient fixtures of the REFERENCE MemoryModel('TGN') (models/MemoryModel.py) for the training path: tests/golden/grads_tgn_<case>.npz.
Run where the reference is importable (the build container), like oracle/make_golden.py, whose reference bindings it reuses:

    python tools/make_golden_tgn_grads.py          # writes tests/golden/grads_tgn_*.npz

Per gc.TGN_CASES case: the reference in eval mode (dropout is the identity), memory bank initialised; every batch but the last under no_grad
(negative call, then positive call), so that the last batch meets real pending messages; on the last batch both calls with autograd,
loss = sum(neg_src G1) + sum(neg_dst G2) + sum(pos_src G2) + sum(pos_dst G1) (G1, G2 = gc.grad_loss_weights(B)), loss.backward().  Stored:
the loss, the four embedding blocks, the final memory bank, every parameter gradient through gc.grad_signature and the names of the
parameters that received one (the memory bank's do not).  grads_tgn_uniform_tgn_bip_l1_k10.npz: the same on a `uniform` sampler
(gc.SAMPLING_STRATEGIES["uniform"]) from the first batch on.  Only outputs are stored; the inputs are rebuilt from the recipes.

While generating, the tool checks what makes the fixtures worth having: the GRUCell weights get non-zero gradients in every file, some node id
sits at more than one level-0 position (its feature-row gradient is a sum) in every file, and at least one file has level-0 entries both with
and without a pending message.  It prints the counts."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as mg          # noqa: E402  (binds the reference classes)
from tests import golden_cases as gc          # noqa: E402

UNIFORM_CASE = "tgn_bip_l1_k10"


def _model(c, strategy="recent", seed=1, tsf=0.0):
    d, cfg = c["data"], c["tgn_cfg"]
    ref_data = mg.RefData(d.src_node_ids, d.dst_node_ids, d.node_interact_times, d.edge_ids, d.labels)
    sampler = mg.ref_get_neighbor_sampler(ref_data, sample_neighbor_strategy=strategy, time_scaling_factor=tsf, seed=seed)
    model = mg.RefMemoryModel(c["node_feat"], c["edge_feat"], sampler, time_feat_dim=cfg["time_feat_dim"], model_name="TGN",
                              num_layers=cfg["num_layers"], num_heads=cfg["num_heads"], dropout=0.1, device="cpu")
    sd = model.state_dict()
    for k, v in c["tgn_params"].items():
        assert k in sd and tuple(sd[k].shape) == v.shape, k
        sd[k] = torch.from_numpy(v)
    model.load_state_dict(sd, strict=True)
    model.eval()
    model.memory_bank.__init_memory_bank__()
    return model, ref_data


def _level0_stats(model, ref_data, c, b) -> dict:
    """level-0 entries of the last batch's two calls under `recent` sampling (roots and neighbours down the recursion), split by whether the
    node has a pending raw message when the batch starts"""
    cfg = c["tgn_cfg"]
    probe = mg.ref_get_neighbor_sampler(ref_data, sample_neighbor_strategy="recent", seed=1)
    pending = {n for n, msgs in model.memory_bank.node_raw_messages.items() if len(msgs) > 0}
    out = {}
    for tag, dst in (("neg", b["neg"]), ("pos", b["dst"])):
        ids, ts = np.concatenate([b["src"], dst]), np.concatenate([b["t"], b["t"]])
        roots = ids
        for _ in range(cfg["num_layers"]):
            nb, _, nt = probe.get_historical_neighbors(ids, ts, num_neighbors=cfg["num_neighbors"])
            ids, ts = np.concatenate([ids, nb.reshape(-1)]), np.concatenate([ts, nt.reshape(-1).astype(np.float64)])
        has = np.array([int(n) in pending for n in ids])
        root_has = np.array([int(n) in pending for n in np.unique(roots)])
        _, counts = np.unique(ids[ids != 0], return_counts=True)
        out[tag] = dict(entries=len(ids), with_msg=int(has.sum()), without_msg=int((~has).sum()), roots_with=int(root_has.sum()),
                        roots_without=int((~root_has).sum()), repeated_nodes=int((counts > 1).sum()))
    return out


def run_case(name: str, strategy="recent", seed=1, tsf=0.0):
    c = gc.build_tgn_case(name)
    cfg = c["tgn_cfg"]
    model, ref_data = _model(c, strategy, seed, tsf)
    k = cfg["num_neighbors"]

    def step(b):
        ns, nd = model.compute_src_dst_node_temporal_embeddings(b["src"], b["neg"], b["t"], edge_ids=None, edges_are_positive=False, num_neighbors=k)
        ps, pd = model.compute_src_dst_node_temporal_embeddings(b["src"], b["dst"], b["t"], edge_ids=b["eid"], edges_are_positive=True, num_neighbors=k)
        return ns, nd, ps, pd
    with torch.no_grad():
        for b in c["tgn_batches"][:-1]:
            step(b)
    b = c["tgn_batches"][-1]
    stats = _level0_stats(model, ref_data, c, b)
    ns, nd, ps, pd = step(b)
    G1, G2 = (torch.from_numpy(g) for g in gc.grad_loss_weights(len(b["src"])))
    loss = (ns * G1).sum() + (nd * G2).sum() + (ps * G2).sum() + (pd * G1).sum()
    loss.backward()
    out = {"loss": np.array(float(loss.detach())), "neg_src_emb": ns.detach().numpy(), "neg_dst_emb": nd.detach().numpy(),
           "pos_src_emb": ps.detach().numpy(), "pos_dst_emb": pd.detach().numpy()}
    with_grad = []
    for pname, p in model.named_parameters():
        # (after a positive call under autograd the reference's node_memories is a non-leaf until detach_memory_bank(): it has no .grad)
        if p.is_leaf and p.grad is not None:
            with_grad.append(pname)
            out.update(gc.grad_signature(pname, p.grad.numpy()))
    out["params_with_grad"] = np.array(sorted(with_grad))
    model.memory_bank.detach_memory_bank()
    out["final_memory"] = model.memory_bank.node_memories.data.numpy().copy()
    out["final_last_update"] = model.memory_bank.node_last_updated_times.data.numpy().copy()
    g = dict(model.named_parameters())
    gru = "memory_updater.memory_updater."
    assert float(g[gru + "weight_ih"].grad.abs().max()) > 0 and float(g[gru + "weight_hh"].grad.abs().max()) > 0, "GRUCell got no gradient"
    assert not any("memory_bank" in n for n in with_grad), with_grad
    assert all(s["repeated_nodes"] > 0 for s in stats.values()), stats
    return out, stats


def main():
    torch.set_num_threads(8)
    jobs = [("grads_" + n, n, ("recent", 1, 0.0)) for n in gc.TGN_CASES] + [("grads_tgn_uniform_" + UNIFORM_CASE, UNIFORM_CASE, gc.SAMPLING_STRATEGIES["uniform"])]
    mixed = False
    for fname, case, smp in jobs:
        out, stats = run_case(case, *smp)
        path = os.path.join(gc.GOLDEN_DIR, fname + ".npz")
        np.savez_compressed(path, **out)
        mixed = mixed or any(s["with_msg"] > 0 and s["without_msg"] > 0 for s in stats.values())
        print(f"{fname}: {os.path.getsize(path) / 1024:.1f} KiB  loss {float(out['loss']):.6g}  level-0 (recent) {stats}")
    assert mixed, "no file has level-0 entries both with and without a pending message"


if __name__ == "__main__":
    main()
