"""EdgeBank restated on the CPU with dicts and numpy, independently of the HIP path (reference models/EdgeBank.py:7-121 and the loop at
evaluate_models_utils.py:303-350): the parity baseline of the GPU tests and the timing baseline of tools/bench_edgebank.py.  Like the reference
it rebuilds the memory from the whole history on every call.  repeat_interval uses the telescoped form of the mean of consecutive differences,
(t[last position] - t[first position]) / (n - 1) per pair, positions being history positions (the history need not be chronological)."""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np


def window_start(src: np.ndarray, dst: np.ndarray, times: np.ndarray, time_window_mode: str, time_window_proportion: float) -> float:
    """EdgeBank.py:51-70: the start of the time window over the history (its end is max(times))."""
    if time_window_mode == "fixed_proportion":
        return float(np.quantile(times, 1 - time_window_proportion))
    if time_window_mode != "repeat_interval":
        raise ValueError(f"Not implemented error for time_window_mode {time_window_mode}!")
    first, last, count = {}, {}, {}
    for p, pair in enumerate(zip(src.tolist(), dst.tolist())):
        first.setdefault(pair, p)
        last[pair] = p
        count[pair] = count.get(pair, 0) + 1
    total = 0.0
    for pair, n in count.items():
        if n > 1:
            total += (times[last[pair]] - times[first[pair]]) / (n - 1)
    return float(max(times) - total / len(count))


def edge_memories(src: np.ndarray, dst: np.ndarray, times: np.ndarray, edge_bank_memory_mode: str, time_window_mode: str,
                  time_window_proportion: float) -> set:
    pairs = list(zip(src.tolist(), dst.tolist()))
    if edge_bank_memory_mode == "unlimited_memory":
        return set(pairs)
    if edge_bank_memory_mode == "repeat_threshold_memory":
        count = {}
        for pair in pairs:
            count[pair] = count.get(pair, 0) + 1
        threshold = float(len(pairs)) / float(len(count)) if count else 0.0              # the mean of the counts
        return {pair for pair, n in count.items() if float(n) >= threshold}
    if edge_bank_memory_mode == "time_window_memory":
        if time_window_mode not in ("fixed_proportion", "repeat_interval"):
            raise ValueError(f"Not implemented error for time_window_mode {time_window_mode}!")
        if len(pairs) == 0:
            raise ValueError("max() arg is an empty sequence")
        start = window_start(src, dst, times, time_window_mode, time_window_proportion)
        return {pair for pair, t in zip(pairs, times.tolist()) if t >= start}
    raise ValueError(f"Not implemented error for edge_bank_memory_mode {edge_bank_memory_mode}!")


def edge_bank_link_prediction(history_data, positive_edges: tuple, negative_edges: tuple, edge_bank_memory_mode: str, time_window_mode: str,
                              time_window_proportion: float) -> Tuple[np.ndarray, np.ndarray]:
    memory = edge_memories(np.asarray(history_data.src_node_ids), np.asarray(history_data.dst_node_ids),
                           np.asarray(history_data.node_interact_times, dtype=np.float64), edge_bank_memory_mode, time_window_mode,
                           time_window_proportion)
    score = lambda edges: np.array([1.0 if pair in memory else 0.0 for pair in zip(np.asarray(edges[0]).tolist(), np.asarray(edges[1]).tolist())])
    return score(positive_edges), score(negative_edges)


def bce_loss(predicts: np.ndarray, labels: np.ndarray) -> float:
    """torch.nn.BCELoss (mean; logs clamped at -100) on 0 / 1 scores: 100 per wrong score."""
    with np.errstate(divide="ignore"):
        lp, lq = np.maximum(np.log(predicts), -100.0), np.maximum(np.log(1.0 - predicts), -100.0)
    return float(np.mean(-(labels * lp + (1.0 - labels) * lq)))


def evaluate(src: np.ndarray, dst: np.ndarray, times: np.ndarray, base: int, batches: List[np.ndarray], negatives: List[Tuple[np.ndarray, np.ndarray]],
             edge_bank_memory_mode: str, time_window_mode: str, test_ratio: float, limit: Optional[int] = None) -> List[np.ndarray]:
    """The reference's per-batch rebuild over one edge list (history of a batch = the first base + indices[0] edges, test edge i = edge
    base + i) -> per batch the scores [positives ; negatives]; `limit` stops after that many batches."""
    class H:
        pass
    out = []
    for idx, (neg_src, neg_dst) in list(zip(batches, negatives))[:limit]:
        h = H()
        n = base + int(idx[0])
        h.src_node_ids, h.dst_node_ids, h.node_interact_times = src[:n], dst[:n], times[:n]
        pos, neg = edge_bank_link_prediction(h, (src[base + idx], dst[base + idx]), (neg_src, neg_dst), edge_bank_memory_mode, time_window_mode,
                                             test_ratio)
        out.append(np.concatenate([pos, neg]))
    return out
