"""Recipes of the EdgeBank tests: the inputs are rebuilt from seeds here; tests/golden/edgebank_*.npz (tools/make_golden_edgebank.py) holds only
what the reference computed from them.

Graph cases (CASES): an edge list, a history length, a batch size over the remaining edges, a negative sampler seed.
  bip           bipartite, chronological float times; 180 test edges in batches of 50, so the last batch is ragged
  gen_unsorted  12 nodes, integer times with many ties, self-loops, repeated pairs, a shuffled tail: the one-shot function only
  gen_sorted    the same graph stably sorted by time: the function and the evaluation loop
Hand-made cases (hand_cases()): a few edges each, expected scores derivable on paper."""
from __future__ import annotations

import os

import numpy as np

from dyglib_amd import synthetic as syn
from dyglib_amd.data_loader import Data

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = [("unlimited_memory", "fixed_proportion"), ("repeat_threshold_memory", "fixed_proportion"),
         ("time_window_memory", "fixed_proportion"), ("time_window_memory", "repeat_interval")]
MODE_KEYS = ["unlimited", "threshold", "window_fixed", "window_repeat"]
TEST_RATIO = 0.15               # time_window_proportion (the reference passes args.test_ratio)
MARGIN = 1e-6                   # smallest allowed min |t - start| / span of a window-mode batch (see make_golden_edgebank.py)
CASES = {
    "bip": dict(history=1020, n_train=840, batch=50, neg_seed=2, loop=True),
    "gen_unsorted": dict(history=300, n_train=210, batch=100, neg_seed=2, loop=False),
    "gen_sorted": dict(history=300, n_train=210, batch=37, neg_seed=2, loop=True),
}


def _sub(d, a, b) -> Data:
    return Data(d.src_node_ids[a:b], d.dst_node_ids[a:b], d.node_interact_times[a:b], d.edge_ids[a:b], d.labels[a:b])


def build_case(name: str) -> dict:
    """-> full / train / val / test Data, the batches' index arrays into test, and the recipe."""
    r = CASES[name]
    if name == "bip":
        d, _, _ = syn.make_bipartite_graph(60, 25, 1200, seed=11)
    else:
        d, _, _ = syn.make_general_graph(12, 400, seed=5)
        if name == "gen_sorted":
            o = np.argsort(d.node_interact_times, kind="stable")
            d = syn.InteractionData(d.src_node_ids[o], d.dst_node_ids[o], d.node_interact_times[o], d.edge_ids[o], d.labels[o])
    E, H = d.num_interactions, r["history"]
    batches = [np.arange(a, min(a + r["batch"], E - H)) for a in range(0, E - H, r["batch"])]
    return dict(name=name, full=_sub(d, 0, E), train=_sub(d, 0, r["n_train"]), val=_sub(d, r["n_train"], H), test=_sub(d, H, E), batches=batches, **r)


def history_of(c: dict, batch: int) -> Data:
    """evaluate_models_utils.py:329-333: train ++ val ++ test[:indices[0]]."""
    return _sub(c["full"], 0, c["history"] + int(c["batches"][batch][0]))


def load_golden(name: str):
    return np.load(os.path.join(GOLDEN_DIR, f"edgebank_{name}.npz"))


# ---- hand-made cases ---------------------------------------------------------------------------------------------------------------
def _home_slot(src: int, dst: int, capacity: int) -> int:
    """The hash dyglib_amd/csrc/edgebank.hip documents: MurmurHash3's 64-bit finaliser of (src << 32) | dst, masked."""
    m = (1 << 64) - 1
    k = (src << 32) | dst
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & m
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & m
    k ^= k >> 33
    return k & (capacity - 1)


def colliding_pairs(capacity: int = 16, homes=(15, 15, 15, 14, 14, 15)):
    """The first pairs (ascending src, dst from 1) whose home slots are `homes`, in that order of need: five for a history whose probes
    collide and wrap past the table's end at the minimum capacity of a five-edge table, one more that is never inserted."""
    want, got = list(homes), [None] * len(homes)
    for s in range(1, 200):
        for d in range(1, 200):
            h = _home_slot(s, d, capacity)
            for i, w in enumerate(want):
                if got[i] is None and w == h:
                    got[i] = (s, d)
                    break
            if all(g is not None for g in got):
                return got
    raise AssertionError("no colliding pairs found")


def hand_cases() -> list:
    """dicts: name, history (src, dst, t), queries (src, dst), mode, window_mode, proportion, expected (scores derivable on paper)."""
    f = lambda *rows: tuple(np.array(c, dtype=t) for c, t in zip(zip(*rows), (np.int64, np.int64, np.float64)))
    q = lambda *rows: tuple(np.array(c, dtype=np.int64) for c in zip(*rows))
    cases = [
        # np.quantile([0..4], 0.5) == 2.0 exactly: the edge at t = 2 is inside the window (>=), the one at t = 1 is not
        dict(name="tie_at_start", history=f((1, 2, 0.0), (3, 4, 1.0), (5, 6, 2.0), (7, 8, 3.0), (9, 10, 4.0)),
             queries=q((5, 6), (3, 4), (1, 2), (9, 10)), mode="time_window_memory", window_mode="fixed_proportion", proportion=0.5,
             expected=[1.0, 0.0, 0.0, 1.0]),
        # counts 2, 2: threshold 4 / 2 = 2, both kept (>=)
        dict(name="threshold_all", history=f((1, 2, 0.0), (1, 2, 1.0), (3, 4, 2.0), (3, 4, 3.0)), queries=q((1, 2), (3, 4), (2, 1)),
             mode="repeat_threshold_memory", window_mode="fixed_proportion", proportion=0.15, expected=[1.0, 1.0, 0.0]),
        # counts 2, 1: threshold 3 / 2 = 1.5, only (1, 2) kept
        dict(name="threshold_one", history=f((1, 2, 0.0), (1, 2, 1.0), (3, 4, 2.0)), queries=q((1, 2), (3, 4)),
             mode="repeat_threshold_memory", window_mode="fixed_proportion", proportion=0.15, expected=[1.0, 0.0]),
        # directed pairs, a self-loop, node id 0 on either side
        dict(name="direction_selfloop_zero", history=f((1, 2, 0.0), (3, 3, 1.0), (0, 5, 2.0), (6, 0, 3.0), (0, 0, 4.0)),
             queries=q((1, 2), (2, 1), (3, 3), (0, 5), (5, 0), (6, 0), (0, 6), (0, 0), (0, 3), (3, 0)),
             mode="unlimited_memory", window_mode="fixed_proportion", proportion=0.15,
             expected=[1.0, 0.0, 1.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0]),
        # repeat_interval on paper: (1,2) at t = 0, 4, 10 -> mean interval 5; (3,4) once; D = 2, S = 5, start = 10 - 2.5 = 7.5:
        # (1,2) (max time 10) is inside, (3,4) (time 7) is not
        dict(name="repeat_interval", history=f((1, 2, 0.0), (1, 2, 4.0), (3, 4, 7.0), (1, 2, 10.0)), queries=q((1, 2), (3, 4)),
             mode="time_window_memory", window_mode="repeat_interval", proportion=0.15, expected=[1.0, 0.0]),
    ]
    # five keys with home slots 15, 15, 15, 14, 14 in the 16 slots of a five-edge table: probes collide and wrap to slots 0, 1, 2; the sixth
    # pair (home 15) was never inserted: its probe walks the whole cluster across the table's end and stops at the first empty slot
    p = colliding_pairs()
    assert [_home_slot(s, d, 16) for s, d in p] == [15, 15, 15, 14, 14, 15]
    cases.append(dict(name="collisions_wrap", history=f(*[(s, d, float(i)) for i, (s, d) in enumerate(p[:5])]),
                      queries=q(*p, *[(d, s) for s, d in p[:2]]), mode="unlimited_memory", window_mode="fixed_proportion", proportion=0.15,
                      expected=[1.0] * 5 + [0.0] + [0.0, 0.0]))
    # one pair 300 times and another 299 times in a single insert range (more than one workgroup of concurrent atomics on one slot):
    # threshold 599 / 2 = 299.5 separates count 300 from count 299
    cases.append(dict(name="duplicates", history=f(*([(7, 9, 1.0)] * 300 + [(8, 9, 2.0)] * 299)), queries=q((7, 9), (8, 9), (9, 7)),
                      mode="repeat_threshold_memory", window_mode="fixed_proportion", proportion=0.15, expected=[1.0, 0.0, 0.0]))
    return cases
