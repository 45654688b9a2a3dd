"""Fixtures of the JODIE and DyRep tests, produced by the REFERENCE itself: imports it from $DYGLIB_REFERENCE at run time (nothing of it is copied), loads
the seeded parameters of tests/memory_variant_cases.py with strict=True, runs the eval-mode model on the CPU and writes

    tests/golden/<case>.npz       per batch the four embedding blocks (negative call, then positive call: b<i>_neg_src / _neg_dst / _pos_src /
                                  _pos_dst), the final memory and last-update tables, the state_dict key list, and the four time-shift
                                  constants of the reference's compute_src_dst_node_time_shifts on the case's training split
    tests/golden/dyrep_<case>[_<tag>].npz   the same blocks and tables for DyRep: `recent` sampling, and one file per random-strategy tag
    tests/golden/eval_jodie.npz, eval_dyrep.npz   per-batch loss / AP / AUC of the reference's evaluate_model_link_prediction("JODIE", ...) and its negative draws

Only outputs are stored; the tests rebuild the inputs from the recipes.  The files are byte-reproducible (fixed zip timestamps).

    DYGLIB_REFERENCE=<reference checkout> python tools/make_golden_memory_variants.py
"""
from __future__ import annotations

import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = os.environ.get("DYGLIB_REFERENCE")
if not REF or not os.path.isdir(REF):
    raise SystemExit("set DYGLIB_REFERENCE to a checkout of the reference (DyGLib): this tool imports it to produce the fixtures")
sys.path.insert(0, REF)

from tests import golden_cases as gc  # noqa: E402
from tests import memory_variant_cases as mv  # noqa: E402


def save(path: str, arrays: dict):
    """np.savez_compressed with a fixed member order and timestamp: the same bytes on every run"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(f"{path}: {os.path.getsize(path)} bytes")


def ref_model(c):
    from models.MemoryModel import MemoryModel
    m = MemoryModel(c["node_feat"], c["edge_feat"], None, mv.TIME_FEAT_DIM, model_name="JODIE", num_layers=1, num_heads=2, dropout=0.1,
                    **mv.model_kwargs(c))
    sd = m.state_dict()
    sd.update({k: torch.from_numpy(v) for k, v in c["params"].items()})
    m.load_state_dict(sd, strict=True)
    return m.eval()


def make_case(name: str):
    from models.MemoryModel import compute_src_dst_node_time_shifts
    c = mv.build_case(name)
    n = c["n_train"]
    shifts = compute_src_dst_node_time_shifts(c["src"][:n], c["dst"][:n], c["t"][:n])
    assert tuple(float(x) for x in shifts) == c["shifts"]
    m = ref_model(c)
    out = {"state_dict_keys": np.array(sorted(m.state_dict().keys())), "time_shifts": np.array(shifts, dtype=np.float64)}
    m.memory_bank.__init_memory_bank__()
    with torch.no_grad():
        for i, b in enumerate(c["batches"]):
            ns, nd = m.compute_src_dst_node_temporal_embeddings(b["src"], b["neg"], b["t"], None, edges_are_positive=False)
            ps, pd = m.compute_src_dst_node_temporal_embeddings(b["src"], b["dst"], b["t"], b["eid"], edges_are_positive=True)
            for tag, v in (("neg_src", ns), ("neg_dst", nd), ("pos_src", ps), ("pos_dst", pd)):
                out[f"b{i}_{tag}"] = v.numpy().copy()
    out["final_memory"] = m.memory_bank.node_memories.data.numpy().copy()
    out["final_last_update"] = m.memory_bank.node_last_updated_times.data.numpy().copy()
    last = len(c["batches"]) - 1
    print(f"{name}: shifts {shifts}, max |emb| {np.abs(out[f'b{last}_pos_src']).max():.3g}, max |memory| {np.abs(out['final_memory']).max():.3g}")
    save(os.path.join(gc.GOLDEN_DIR, f"{name}.npz"), out)


def make_eval():
    from evaluate_models_utils import evaluate_model_link_prediction
    from models.modules import MergeLayer
    from utils.DataLoader import Data, get_idx_data_loader
    from utils.utils import NegativeEdgeSampler
    r = mv.EVAL_CASE
    c = mv.build_case(r["case"])
    backbone = ref_model(c)
    merge = MergeLayer(172, 172, 172, 1)
    merge.load_state_dict({k: torch.from_numpy(v) for k, v in c["mparams"].items()}, strict=True)
    model = torch.nn.Sequential(backbone, merge)
    a, b = gc.eval_indices(len(c["src"]))
    ev = Data(c["src"][a:b], c["dst"][a:b], c["t"][a:b], c["eid"][a:b], c["labels"][a:b])
    neg = NegativeEdgeSampler(c["src"], c["dst"], seed=gc.EVAL_NEG_SEED)
    loader = get_idx_data_loader(list(range(b - a)), batch_size=r["batch"], shuffle=False)
    backbone.memory_bank.__init_memory_bank__()
    losses, metrics = evaluate_model_link_prediction("JODIE", model, None, loader, neg, ev, torch.nn.BCELoss())
    neg.reset_random_state()
    draws = np.concatenate([neg.sample(size=len(idx))[1] for idx in loader])
    save(os.path.join(gc.GOLDEN_DIR, "eval_jodie.npz"),
         dict(losses=np.array(losses, dtype=np.float64), average_precision=np.array([m["average_precision"] for m in metrics]),
              roc_auc=np.array([m["roc_auc"] for m in metrics]), neg_dst=draws.astype(np.int64)))
    print(f"eval_jodie: {len(losses)} batches, losses {np.round(losses[:3], 4)}")


def ref_dyrep(c, strategy="recent", seed=1, tsf=0.0):
    from models.MemoryModel import MemoryModel
    from utils.DataLoader import Data
    from utils.utils import get_neighbor_sampler
    d, cfg = c["data"], c["cfg"]
    sampler = get_neighbor_sampler(Data(d.src_node_ids, d.dst_node_ids, d.node_interact_times, d.edge_ids, d.labels), sample_neighbor_strategy=strategy,
                                   time_scaling_factor=tsf, seed=seed)
    m = MemoryModel(c["node_feat"], c["edge_feat"], sampler, cfg["time_feat_dim"], model_name="DyRep", num_layers=cfg["num_layers"],
                    num_heads=cfg["num_heads"], dropout=0.1)
    sd = m.state_dict()
    sd.update({k: torch.from_numpy(v) for k, v in c["params"].items()})
    m.load_state_dict(sd, strict=True)
    return m.eval(), sampler


def make_dyrep_case(name: str):
    c = mv.build_dyrep_case(name)
    k = c["cfg"]["num_neighbors"]
    runs = [("", ("recent", 1, 0.0))] + [("_" + tag, gc.SAMPLING_STRATEGIES[tag]) for tag in mv.DYREP_RANDOM_TAGS]
    for suffix, (strategy, seed, tsf) in runs:
        m, sampler = ref_dyrep(c, strategy, seed, tsf)
        out = {"state_dict_keys": np.array(sorted(m.state_dict().keys()))} if not suffix else {}
        m.set_neighbor_sampler(sampler)
        m.memory_bank.__init_memory_bank__()
        with torch.no_grad():
            for i, b in enumerate(c["batches"]):
                ns, nd = m.compute_src_dst_node_temporal_embeddings(b["src"], b["neg"], b["t"], None, edges_are_positive=False, num_neighbors=k)
                ps, pd = m.compute_src_dst_node_temporal_embeddings(b["src"], b["dst"], b["t"], b["eid"], edges_are_positive=True, num_neighbors=k)
                for tag, v in (("neg_src", ns), ("neg_dst", nd), ("pos_src", ps), ("pos_dst", pd)):
                    out[f"b{i}_{tag}"] = v.numpy().copy()
        out["final_memory"] = m.memory_bank.node_memories.data.numpy().copy()
        out["final_last_update"] = m.memory_bank.node_last_updated_times.data.numpy().copy()
        print(f"{name}{suffix}: max |memory| {np.abs(out['final_memory']).max():.3g}")
        save(os.path.join(gc.GOLDEN_DIR, f"{name}{suffix}.npz"), out)


def make_dyrep_eval():
    from evaluate_models_utils import evaluate_model_link_prediction
    from models.modules import MergeLayer
    from utils.DataLoader import Data, get_idx_data_loader
    from utils.utils import NegativeEdgeSampler
    r = mv.DYREP_EVAL_CASE
    c = mv.build_dyrep_case(r["case"])
    backbone, sampler = ref_dyrep(c)
    merge = MergeLayer(172, 172, 172, 1)
    merge.load_state_dict({k: torch.from_numpy(v) for k, v in c["mparams"].items()}, strict=True)
    model = torch.nn.Sequential(backbone, merge)
    d = c["data"]
    a, b = gc.eval_indices(d.num_interactions)
    ev = Data(d.src_node_ids[a:b], d.dst_node_ids[a:b], d.node_interact_times[a:b], d.edge_ids[a:b], d.labels[a:b])
    neg = NegativeEdgeSampler(d.src_node_ids, d.dst_node_ids, seed=gc.EVAL_NEG_SEED)
    loader = get_idx_data_loader(list(range(b - a)), batch_size=r["batch"], shuffle=False)
    backbone.memory_bank.__init_memory_bank__()
    losses, metrics = evaluate_model_link_prediction("DyRep", model, sampler, loader, neg, ev, torch.nn.BCELoss(), num_neighbors=c["cfg"]["num_neighbors"])
    neg.reset_random_state()
    draws = np.concatenate([neg.sample(size=len(idx))[1] for idx in loader])
    save(os.path.join(gc.GOLDEN_DIR, "eval_dyrep.npz"),
         dict(losses=np.array(losses, dtype=np.float64), average_precision=np.array([m["average_precision"] for m in metrics]),
              roc_auc=np.array([m["roc_auc"] for m in metrics]), neg_dst=draws.astype(np.int64)))


if __name__ == "__main__":
    which = sys.argv[1:] or ["jodie", "dyrep"]
    if "jodie" in which:
        for name in mv.CASES:
            make_case(name)
        make_eval()
    if "dyrep" in which:
        for name in mv.DYREP_CASES:
            make_dyrep_case(name)
        make_dyrep_eval()
