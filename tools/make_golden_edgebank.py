"""Fixtures of the EdgeBank tests, produced by the REFERENCE itself: imports it from $DYGLIB_REFERENCE at run time (nothing of it is copied) and
drives its own edge_bank_link_prediction, NegativeEdgeSampler, get_link_prediction_metrics and BCELoss over the recipes of
tests/edgebank_cases.py, batch by batch as evaluate_models_utils.py:303-350 does.  Only outputs are stored:

    tests/golden/edgebank_<case>.npz   neg_dst (the sampler's draws, all batches) and, per mode combination <m> of edgebank_cases.MODE_KEYS,
                                       <m>|prob (per batch [positives ; negatives], concatenated), <m>|loss, <m>|average_precision, <m>|roc_auc
                                       [n_batches] and, for the window modes, <m>|start (the reference's own time_window_start_time, read from
                                       its frame when edge_bank_time_window_memory returns) and <m>|gap = min |t - start| / span over the
                                       history times of the batch
    tests/golden/edgebank_hand.npz     <name>|prob of every hand-made case (and |start for the window ones)

Margin condition of the window modes.  repeat_interval is computed here and in the oracle from the telescoped sum, which is not bit-identical
to the reference's sum of np.mean's: a float64 sum of at most 1e5 terms is off by about 1e-11 relative, so a history time within that of
`start` could flip a score.  A graph case whose gap is below edgebank_cases.MARGIN = 1e-6 (five orders of headroom) is rejected here, and the
tests assert the stored gaps against the same bound.  The hand-made cases use small integers, where both sums are exact (one of them puts a
time exactly on `start` on purpose).

The files are written with fixed zip timestamps, so a rerun reproduces them byte for byte.

    DYGLIB_REFERENCE=<checkout of the reference> python tools/make_golden_edgebank.py
"""
from __future__ import annotations

import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if "DYGLIB_REFERENCE" not in os.environ:
    sys.exit("set DYGLIB_REFERENCE to a checkout of the reference")
sys.path.insert(0, os.environ["DYGLIB_REFERENCE"])

from tests import edgebank_cases as ec  # noqa: E402


def save_npz(path: str, arrays: dict) -> None:
    """np.savez_compressed with a fixed member timestamp and order."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[key]), allow_pickle=False)
    print(f"{path}: {os.path.getsize(path)} bytes")


def reference_scores(history, pos, neg, mode, window_mode, proportion):
    """The reference's edge_bank_link_prediction and, for time_window_memory, the time_window_start_time it used (a local of its
    edge_bank_time_window_memory, read when that frame returns)."""
    from models.EdgeBank import edge_bank_link_prediction
    from utils.DataLoader import Data
    seen = {}

    def profile(frame, event, arg):
        if event == "return" and frame.f_code.co_name == "edge_bank_time_window_memory":
            seen["start"] = float(frame.f_locals["time_window_start_time"])

    h = Data(history.src_node_ids, history.dst_node_ids, history.node_interact_times, history.edge_ids, history.labels)
    sys.setprofile(profile)
    try:
        p, n = edge_bank_link_prediction(h, pos, neg, mode, window_mode, proportion)
    finally:
        sys.setprofile(None)
    return p, n, seen.get("start")


def make_case(name: str) -> None:
    from utils.metrics import get_link_prediction_metrics
    from utils.utils import NegativeEdgeSampler
    c = ec.build_case(name)
    full, test = c["full"], c["test"]
    sampler = NegativeEdgeSampler(full.src_node_ids, full.dst_node_ids, seed=c["neg_seed"])
    sampler.reset_random_state()
    negs = [sampler.sample(size=len(idx))[1] for idx in c["batches"]]
    out = {"neg_dst": np.concatenate(negs).astype(np.int64)}
    loss_func = torch.nn.BCELoss()
    for key, (mode, window_mode) in zip(ec.MODE_KEYS, ec.MODES):
        probs, losses, aps, aucs, starts, gaps = [], [], [], [], [], []
        for b, idx in enumerate(c["batches"]):
            hist = ec.history_of(c, b)
            src = test.src_node_ids[idx]
            p, n, start = reference_scores(hist, (src, test.dst_node_ids[idx]), (src, negs[b]), mode, window_mode, ec.TEST_RATIO)
            assert 0 < p.sum() < len(p) and 0 < n.sum() < len(n), (name, key, b, "a batch with trivial scores")
            predicts = torch.from_numpy(np.concatenate([p, n])).float()                                   # evaluate_models_utils.py:343-350
            labels = torch.cat([torch.ones(len(p)), torch.zeros(len(n))], dim=0)
            losses.append(loss_func(input=predicts, target=labels).item())
            m = get_link_prediction_metrics(predicts=predicts, labels=labels)
            aps.append(m["average_precision"]), aucs.append(m["roc_auc"])
            probs.append(np.concatenate([p, n]))
            if start is not None:
                t = hist.node_interact_times
                gap = float(np.min(np.abs(t - start)) / (t.max() - t.min()))
                if gap < ec.MARGIN:
                    sys.exit(f"{name} {key} batch {b}: a history time lies within {gap:.3g} of the window start (bound {ec.MARGIN}): rejected")
                starts.append(start), gaps.append(gap)
        out[f"{key}|prob"] = np.concatenate(probs).astype(np.float64)
        out[f"{key}|loss"] = np.array(losses, dtype=np.float64)
        out[f"{key}|average_precision"] = np.array(aps, dtype=np.float64)
        out[f"{key}|roc_auc"] = np.array(aucs, dtype=np.float64)
        if starts:
            out[f"{key}|start"], out[f"{key}|gap"] = np.array(starts), np.array(gaps)
            print(f"{name} {key}: smallest gap {min(gaps):.3g}")
    save_npz(os.path.join(ec.GOLDEN_DIR, f"edgebank_{name}.npz"), out)


def make_hand() -> None:
    from dyglib_amd.data_loader import Data
    out = {}
    for h in ec.hand_cases():
        s, d, t = h["history"]
        hist = Data(s, d, t, np.arange(1, len(s) + 1), np.zeros(len(s)))
        empty = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
        p, _, start = reference_scores(hist, h["queries"], empty, h["mode"], h["window_mode"], h["proportion"])
        assert p.tolist() == h["expected"], (h["name"], p.tolist(), h["expected"])          # the paper values are the reference's
        out[f"{h['name']}|prob"] = p.astype(np.float64)
        if start is not None:
            out[f"{h['name']}|start"] = np.array([start])
    save_npz(os.path.join(ec.GOLDEN_DIR, "edgebank_hand.npz"), out)


if __name__ == "__main__":
    for case in ec.CASES:
        make_case(case)
    make_hand()
