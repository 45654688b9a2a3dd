"""EdgeBank, the non-parametric link-prediction baseline (reference models/EdgeBank.py:7-121 and its evaluation loop,
evaluate_models_utils.py:303-350), on a persistent hash table on the GPU (dyglib_amd/csrc/edgebank.hip).

    from dyglib_amd import edge_bank_link_prediction, evaluate_edge_bank_link_prediction      # instead of models.EdgeBank / evaluate_models_utils

`edge_bank_link_prediction` has the reference's signature and result.  The reference's loop rebuilds a Python set over train ++ val ++ the
test prefix for every batch; here every batch's history is a prefix of one chronological edge list, so the table only takes the batch's new
edges, the scores go straight into the metrics kernel, and the host synchronises once, at the end.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _capi
from .evaluate import _is_plain_bce
from .metrics import link_prediction_metrics_device

MEMORY_MODES = {"unlimited_memory": 0, "repeat_threshold_memory": 1, "time_window_memory": 2}
WINDOW_MODES = {"fixed_proportion": 0, "repeat_interval": 1}
ID_LIMIT = 1 << 31
FLAG_MESSAGES = {1: "a node id outside [0, 2^31) reached the kernels", 2: "the table was filled beyond max_edges",
                 4: "an inserted pair was not found again"}
_MASK64 = (1 << 64) - 1


def home_slot(src: int, dst: int, capacity: int) -> int:
    """Home slot of the pair (src, dst) in a table of `capacity` slots (a power of two), as dyglib_amd/csrc/edgebank.hip documents it:
    MurmurHash3's 64-bit finaliser of the key (src << 32) | dst, masked.  Probing then goes (slot + 1) & (capacity - 1)."""
    k = ((int(src) << 32) | int(dst)) & _MASK64
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & _MASK64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & _MASK64
    k ^= k >> 33
    return k & (capacity - 1)


def table_capacity(max_edges: int) -> int:
    """Slots of a table for `max_edges` edges: the power of two >= max(2 * max_edges, 8)."""
    c = 8
    while c < 2 * max_edges:
        c <<= 1
    return c


def _modes(edge_bank_memory_mode: str, time_window_mode: str) -> Tuple[int, int]:
    if edge_bank_memory_mode not in MEMORY_MODES:
        raise ValueError(f"Not implemented error for edge_bank_memory_mode {edge_bank_memory_mode}!")                 # EdgeBank.py:116
    mode = MEMORY_MODES[edge_bank_memory_mode]
    if mode != 2:
        return mode, 0                                                      # the reference looks at time_window_mode in this mode only
    if time_window_mode not in WINDOW_MODES:
        raise ValueError(f"Not implemented error for time_window_mode {time_window_mode}!")                           # EdgeBank.py:70
    return mode, WINDOW_MODES[time_window_mode]


def window_start_time(history_times: np.ndarray, time_window_proportion: float) -> float:
    """fixed_proportion's window start (EdgeBank.py:52), by numpy itself on the host: its interpolation is not restated anywhere."""
    return float(np.quantile(history_times, 1 - time_window_proportion))


def _check_ids(*arrays) -> None:
    for a in arrays:
        if len(a) == 0:
            continue
        lo, hi = int(np.min(a)), int(np.max(a))
        if lo < 0:
            raise ValueError(f"EdgeBank: node id {lo} is outside [0, 2^31)")
        if hi >= ID_LIMIT:
            raise ValueError(f"EdgeBank: node id {hi} is outside [0, 2^31)")


def _ids(a) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype.kind not in "iu":
        if a.size and not np.all(np.asarray(a, dtype=np.float64) == np.floor(np.asarray(a, dtype=np.float64))):
            raise ValueError("EdgeBank: node ids must be integers")
    return np.ascontiguousarray(a, dtype=np.int64).reshape(-1)


def _require_gpu() -> torch.device:
    if not torch.cuda.is_available():
        raise _capi.DygnnError("EdgeBank runs on the GPU only (no device is available)")
    return torch.device("cuda", torch.cuda.current_device())


class EdgeBankTable:
    """The table of dygnn_edgebank_* over one edge list on the device.  `src`, `dst` (int64) and `times` (float64) are the whole list; the
    table holds its first `num_edges` edges."""

    def __init__(self, src: np.ndarray, dst: np.ndarray, times: np.ndarray, device: Optional[torch.device] = None):
        device = device or _require_gpu()
        self.lib = _capi.load()
        self.max_edges = len(src)
        nbytes = self.lib.dygnn_edgebank_table_bytes(self.max_edges)
        if nbytes == 0:
            raise ValueError(f"EdgeBank: {self.max_edges} edges exceed the table's limit of 2^30")
        self.src = torch.from_numpy(np.ascontiguousarray(src, dtype=np.int64)).to(device)
        self.dst = torch.from_numpy(np.ascontiguousarray(dst, dtype=np.int64)).to(device)
        self.times = torch.from_numpy(np.ascontiguousarray(times, dtype=np.float64)).to(device)
        self.buffer = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.c = _capi.EdgeBank(self.buffer.data_ptr(), nbytes, self.max_edges, 0)
        self.reset()

    @property
    def num_edges(self) -> int:
        return int(self.c.num_edges)

    def reset(self) -> None:
        _capi.check(self.lib.dygnn_edgebank_reset(C.byref(self.c), _capi.current_stream_ptr()), ValueError)

    def insert_until(self, last: int) -> None:
        _capi.check(self.lib.dygnn_edgebank_insert(C.byref(self.c), self.src.data_ptr(), self.dst.data_ptr(), self.times.data_ptr(),
                                                   self.num_edges, last, _capi.current_stream_ptr()), ValueError)

    def query(self, mode: int, window_mode: int, start_time: float, q_src: torch.Tensor, q_dst: torch.Tensor) -> torch.Tensor:
        out = torch.empty(q_src.numel(), dtype=torch.float32, device=q_src.device)
        _capi.check(self.lib.dygnn_edgebank_query(C.byref(self.c), self.times.data_ptr(), mode, window_mode, self.num_edges, float(start_time),
                                                  q_src.data_ptr(), q_dst.data_ptr(), q_src.numel(), out.data_ptr(),
                                                  _capi.current_stream_ptr()), ValueError)
        return out

    def evaluate(self, hist_len: np.ndarray, start_times: Optional[torch.Tensor], q_src: torch.Tensor, q_dst: torch.Tensor, mode: int,
                 window_mode: int) -> torch.Tensor:
        """q_src / q_dst: [n_batches, queries_per_batch] int64 on the device -> float32 scores of the same shape; nothing synchronises."""
        n, q = q_src.shape
        hist_len = np.ascontiguousarray(hist_len, dtype=np.int64)
        out = torch.empty((n, q), dtype=torch.float32, device=q_src.device)
        _capi.check(self.lib.dygnn_edgebank_evaluate(C.byref(self.c), self.src.data_ptr(), self.dst.data_ptr(), self.times.data_ptr(),
                                                     hist_len.ctypes.data_as(_capi.c_i64p), _capi.ptr(start_times), q_src.data_ptr(),
                                                     q_dst.data_ptr(), n, q, mode, window_mode, out.data_ptr(), _capi.current_stream_ptr()),
                    ValueError)
        return out

    def flags(self) -> torch.Tensor:
        """The kernels' guard word (int32, on the device): 0 unless something `FLAG_MESSAGES` names happened."""
        return self.buffer[32:36].view(torch.int32)


def _raise_on_flags(flags: int) -> None:
    if flags:
        raise _capi.DygnnError("EdgeBank: " + "; ".join(m for b, m in FLAG_MESSAGES.items() if flags & b))


def edge_bank_link_prediction(history_data, positive_edges: tuple, negative_edges: tuple, edge_bank_memory_mode: str,
                              time_window_mode: str, time_window_proportion: float) -> Tuple[np.ndarray, np.ndarray]:
    """EdgeBank.py:94-121: (positive_probabilities, negative_probabilities), float64 arrays of 0.0 / 1.0, for edges (src_node_ids,
    dst_node_ids) against `history_data` (any object with src_node_ids, dst_node_ids, node_interact_times; any order).  One table build and
    one query call."""
    mode, window_mode = _modes(edge_bank_memory_mode, time_window_mode)
    h_src, h_dst = _ids(history_data.src_node_ids), _ids(history_data.dst_node_ids)
    h_t = np.ascontiguousarray(history_data.node_interact_times, dtype=np.float64).reshape(-1)
    pos_src, pos_dst = _ids(positive_edges[0]), _ids(positive_edges[1])
    neg_src, neg_dst = _ids(negative_edges[0]), _ids(negative_edges[1])
    n_pos, n_neg = len(pos_src), len(neg_src)
    if len(pos_dst) != n_pos or len(neg_dst) != n_neg or len(h_dst) != len(h_src) or len(h_t) != len(h_src):
        raise ValueError("EdgeBank: source, destination and time arrays must have equal lengths")
    H = len(h_src)
    if mode == 2 and H == 0:
        raise ValueError("max() arg is an empty sequence")                                                            # EdgeBank.py:53 / :67
    _check_ids(h_src, h_dst, pos_src, pos_dst, neg_src, neg_dst)
    start = window_start_time(h_t, time_window_proportion) if (mode == 2 and window_mode == 0) else 0.0
    device = _require_gpu()
    if n_pos + n_neg == 0:
        return np.zeros(0), np.zeros(0)
    table = EdgeBankTable(h_src, h_dst, h_t, device)
    table.insert_until(H)
    q_src = torch.from_numpy(np.concatenate([pos_src, neg_src])).to(device)
    q_dst = torch.from_numpy(np.concatenate([pos_dst, neg_dst])).to(device)
    out = table.query(mode, window_mode, start, q_src, q_dst)
    host = torch.cat([out, table.flags().float()]).cpu().numpy()                    # the only synchronisation
    _raise_on_flags(int(host[-1]))
    prob = host[:-1].astype(np.float64)
    return prob[:n_pos], prob[n_pos:]


def edge_bank_scores(train_data, val_data, test_idx_data_loader, test_neg_edge_sampler, test_data, edge_bank_memory_mode: str,
                     time_window_mode: str, test_ratio: float) -> Tuple[List[torch.Tensor], Optional[EdgeBankTable]]:
    """The scoring half of the evaluation loop: -> (one float32 device tensor [n, 2B] of [positives ; negatives] scores per run of n equally
    sized batches, the table).  Nothing synchronises."""
    mode, window_mode = _modes(edge_bank_memory_mode, time_window_mode)
    assert test_neg_edge_sampler.seed is not None                                                                     # :303
    test_neg_edge_sampler.reset_random_state()
    src = np.concatenate([_ids(d.src_node_ids) for d in (train_data, val_data, test_data)])
    dst = np.concatenate([_ids(d.dst_node_ids) for d in (train_data, val_data, test_data)])
    times = np.concatenate([np.asarray(d.node_interact_times, dtype=np.float64).reshape(-1) for d in (train_data, val_data, test_data)])
    if len(times) > 1 and np.any(np.diff(times) < 0):
        k = int(np.argmax(np.diff(times) < 0))
        raise ValueError(f"EdgeBank evaluation needs chronological data: time {times[k + 1]} at position {k + 1} of train ++ val ++ test "
                         f"follows {times[k]}")
    _check_ids(src, dst)
    base = len(train_data.src_node_ids) + len(val_data.src_node_ids)
    random_negatives = test_neg_edge_sampler.negative_sample_strategy == "random"

    # host pass: negatives in the reference's draw order, history lengths, fixed_proportion starts (np.quantile, once per batch)
    batches = []                                                        # (q_src [2B], q_dst [2B], H, start)
    for test_data_indices in test_idx_data_loader:
        idx = test_data_indices.numpy() if isinstance(test_data_indices, torch.Tensor) else np.asarray(test_data_indices)
        b_src, b_dst = _ids(test_data.src_node_ids[idx]), _ids(test_data.dst_node_ids[idx])
        if random_negatives:                                                                                          # :321-323
            _, neg_dst = test_neg_edge_sampler.sample(size=len(b_src))
            neg_src = b_src
        else:                                                                                                         # :315-320
            b_t = test_data.node_interact_times[idx]
            neg_src, neg_dst = test_neg_edge_sampler.sample(size=len(b_src), batch_src_node_ids=b_src, batch_dst_node_ids=b_dst,
                                                            current_batch_start_time=b_t[0], current_batch_end_time=b_t[-1])
        neg_src, neg_dst = _ids(neg_src), _ids(neg_dst)
        _check_ids(neg_src, neg_dst)
        H = base + int(idx[0])
        if batches and H < batches[-1][2]:
            raise ValueError("EdgeBank evaluation needs the test batches in order: a batch starts before its predecessor")
        start = 0.0
        if mode == 2:
            if H == 0:
                raise ValueError("max() arg is an empty sequence")                                                    # EdgeBank.py:53 / :67
            if window_mode == 0:
                start = window_start_time(times[:H], test_ratio)
        batches.append((np.concatenate([b_src, neg_src]), np.concatenate([b_dst, neg_dst]), H, start))
    if not batches:
        return [], None

    device = _require_gpu()
    table = EdgeBankTable(src, dst, times, device)
    scores = []
    lo = 0
    while lo < len(batches):                                            # runs of equally sized batches (the last one may be ragged): one call each
        hi = lo
        while hi < len(batches) and len(batches[hi][0]) == len(batches[lo][0]):
            hi += 1
        group = batches[lo:hi]
        q_src = torch.from_numpy(np.stack([g[0] for g in group])).to(device)
        q_dst = torch.from_numpy(np.stack([g[1] for g in group])).to(device)
        starts = torch.tensor([g[3] for g in group], dtype=torch.float64).to(device) if (mode == 2 and window_mode == 0) else None
        scores.append(table.evaluate(np.array([g[2] for g in group], dtype=np.int64), starts, q_src, q_dst, mode, window_mode))
        lo = hi
    return scores, table


def evaluate_edge_bank_link_prediction(train_data, val_data, test_idx_data_loader, test_neg_edge_sampler, test_data,
                                       edge_bank_memory_mode: str = "unlimited_memory", time_window_mode: str = "fixed_proportion",
                                       test_ratio: float = 0.15, loss_func: Optional[nn.Module] = None) -> Tuple[List[float], List[dict]]:
    """evaluate_models_utils.py:303-350 (the body of the reference's evaluate_edge_bank_link_prediction, which takes an `args` namespace, logs
    and returns nothing): returns (test_losses, test_metrics), one float and one {'average_precision', 'roc_auc'} dict per batch, like
    evaluate_model_link_prediction.  `loss_func` None = torch.nn.BCELoss() (:297).  The history of a batch is train ++ val ++
    test[:indices[0]] (:329-333); the concatenated times must not decrease, since the table holds prefixes of that one list."""
    scores, table = edge_bank_scores(train_data, val_data, test_idx_data_loader, test_neg_edge_sampler, test_data, edge_bank_memory_mode,
                                     time_window_mode, test_ratio)
    if not scores:
        return [], []
    plain_bce = loss_func is None or _is_plain_bce(loss_func)
    results = []
    for predicts in scores:                                                                       # [positives ; negatives], :343
        n, half = predicts.shape[0], predicts.shape[1] // 2
        labels = torch.cat([torch.ones((n, half), device=predicts.device), torch.zeros((n, half), device=predicts.device)], dim=1)   # :344
        ap, auc, loss, status = link_prediction_metrics_device(predicts, labels)
        if not plain_bce:
            loss = torch.stack([loss_func(input=predicts[i], target=labels[i]).double() for i in range(n)])
        results.append((ap, auc, loss, status.double()))
    results.append(tuple(table.flags().double() for _ in range(4)))
    ap, auc, loss, status = torch.stack([torch.cat([r[i] for r in results]) for i in range(4)]).cpu().numpy()     # the only synchronisation
    _raise_on_flags(int(ap[-1]))
    if status[:-1].any():
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    return [float(v) for v in loss[:-1]], [{"average_precision": float(a), "roc_auc": float(u)} for a, u in zip(ap[:-1], auc[:-1])]
