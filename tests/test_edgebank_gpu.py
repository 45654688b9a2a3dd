"""EdgeBank on the GPU (dyglib_amd/csrc/edgebank.hip behind dyglib_amd/edgebank.py) against the reference's own outputs
(tests/golden/edgebank_*.npz): scores exactly, losses within 1e-5 (the bound of tests/test_evaluate.py), AP / AUC within 1e-12 (the bound
tests/test_metrics.py holds the metrics kernel to), negatives draw for draw.  Shapes are the fixtures' (a few hundred edges: several
workgroups per insert, a ragged last batch) plus the hand-made cases of tests/edgebank_cases.py."""
import functools

import numpy as np
import pytest
import torch

from dyglib_amd import _capi, edgebank as eb
from dyglib_amd.evaluate import NegativeEdgeSampler, get_idx_data_loader
from tests import edgebank_cases as ec
from tests import edgebank_oracle as eo

pytestmark = pytest.mark.gpu
TOL_METRIC = 1e-12
TOL_LOSS = 1e-5
MODE_IDS = list(zip(ec.MODE_KEYS, ec.MODES))


class _Hist:
    def __init__(self, src, dst, t):
        self.src_node_ids, self.dst_node_ids, self.node_interact_times = np.asarray(src), np.asarray(dst), np.asarray(t, dtype=np.float64)


class RecordingSampler(NegativeEdgeSampler):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.draws = []

    def sample(self, size, *a, **k):
        out = super().sample(size, *a, **k)
        self.draws.append(out[1])
        return out


@functools.lru_cache(maxsize=None)
def case(name):
    return ec.build_case(name)


@functools.lru_cache(maxsize=None)
def one_shot(name, key):
    """The one-shot function on every batch of a case: [positives ; negatives] per batch, computed once and shared."""
    c, g = case(name), ec.load_golden(name)
    mode, window_mode = dict(MODE_IDS)[key]
    out, o = [], 0
    for b, idx in enumerate(c["batches"]):
        src = c["test"].src_node_ids[idx]
        p, n = eb.edge_bank_link_prediction(ec.history_of(c, b), (src, c["test"].dst_node_ids[idx]), (src, g["neg_dst"][o:o + len(idx)]), mode,
                                            window_mode, ec.TEST_RATIO)
        assert p.dtype == n.dtype == np.float64 and len(p) == len(n) == len(idx)
        out.append(np.concatenate([p, n]))
        o += len(idx)
    return tuple(out)


def loop_inputs(c):
    sampler = RecordingSampler(c["full"].src_node_ids, c["full"].dst_node_ids, seed=c["neg_seed"])
    loader = get_idx_data_loader(list(range(c["test"].num_interactions)), batch_size=c["batch"], shuffle=False)
    return loader, sampler


@pytest.mark.parametrize("key", ec.MODE_KEYS)
@pytest.mark.parametrize("name", list(ec.CASES))
def test_function_matches_reference_exactly(name, key):
    g = ec.load_golden(name)
    if f"{key}|gap" in g:
        assert (g[f"{key}|gap"] >= ec.MARGIN).all()
    got = np.concatenate(one_shot(name, key))
    assert set(np.unique(got)) <= {0.0, 1.0}
    np.testing.assert_array_equal(got, g[f"{key}|prob"])


@pytest.mark.parametrize("key", ec.MODE_KEYS)
@pytest.mark.parametrize("name", [n for n, r in ec.CASES.items() if r["loop"]])
def test_loop_matches_reference(name, key):
    c, g = case(name), ec.load_golden(name)
    mode, window_mode = dict(MODE_IDS)[key]
    loader, sampler = loop_inputs(c)
    sampler.sample(size=7)                                     # the loop resets the sampler's state, whatever was drawn before
    sampler.draws.clear()
    losses, metrics = eb.evaluate_edge_bank_link_prediction(c["train"], c["val"], loader, sampler, c["test"], edge_bank_memory_mode=mode,
                                                            time_window_mode=window_mode, test_ratio=ec.TEST_RATIO)
    n = len(c["batches"])
    assert len(losses) == len(metrics) == n and all(isinstance(v, float) for v in losses)
    assert len(c["batches"][-1]) < len(c["batches"][0])                                    # the last batch is ragged
    np.testing.assert_array_equal(np.concatenate(sampler.draws), g["neg_dst"])             # draw for draw
    print(name, key, "loss err", np.abs(np.array(losses) - g[f"{key}|loss"]).max(),
          "ap err", np.abs(np.array([m["average_precision"] for m in metrics]) - g[f"{key}|average_precision"]).max(),
          "auc err", np.abs(np.array([m["roc_auc"] for m in metrics]) - g[f"{key}|roc_auc"]).max())
    for b in range(n):
        assert abs(losses[b] - g[f"{key}|loss"][b]) <= TOL_LOSS
        assert set(metrics[b]) == {"average_precision", "roc_auc"}
        assert abs(metrics[b]["average_precision"] - g[f"{key}|average_precision"][b]) <= TOL_METRIC
        assert abs(metrics[b]["roc_auc"] - g[f"{key}|roc_auc"][b]) <= TOL_METRIC
    # a loss function that is not plain mean BCE is applied as given
    loader, sampler = loop_inputs(c)
    sums, _ = eb.evaluate_edge_bank_link_prediction(c["train"], c["val"], loader, sampler, c["test"], edge_bank_memory_mode=mode,
                                                    time_window_mode=window_mode, test_ratio=ec.TEST_RATIO,
                                                    loss_func=torch.nn.BCELoss(reduction="sum"))
    for b in range(n):
        assert abs(sums[b] - g[f"{key}|loss"][b] * 2 * len(c["batches"][b])) <= TOL_LOSS * 2 * len(c["batches"][b])


def loop_scores(c, mode, window_mode):
    loader, sampler = loop_inputs(c)
    scores, table = eb.edge_bank_scores(c["train"], c["val"], loader, sampler, c["test"], mode, window_mode, ec.TEST_RATIO)
    return scores, table


@pytest.mark.parametrize("key", ec.MODE_KEYS)
@pytest.mark.parametrize("name", [n for n, r in ec.CASES.items() if r["loop"]])
def test_incremental_scores_equal_one_shot_calls_and_runs_repeat_bit_for_bit(name, key):
    c = case(name)
    mode, window_mode = dict(MODE_IDS)[key]
    scores, table = loop_scores(c, mode, window_mode)
    assert [tuple(s.shape) for s in scores] == [(len(c["batches"]) - 1, 2 * c["batch"]), (1, 2 * len(c["batches"][-1]))]      # ragged last batch
    assert all(s.dtype == torch.float32 for s in scores)
    flat = [row.cpu().numpy() for s in scores for row in s]
    for b, want in enumerate(one_shot(name, key)):
        np.testing.assert_array_equal(flat[b].astype(np.float64), want)
    assert table.num_edges == c["history"] + int(c["batches"][-1][0]) and int(table.flags().item()) == 0
    # a second run: the same table bytes and the same outputs
    scores2, table2 = loop_scores(c, mode, window_mode)
    assert torch.equal(table.buffer, table2.buffer)
    assert all(torch.equal(a, b) for a, b in zip(scores, scores2))


def _table_of(history):
    s, d, t = history
    table = eb.EdgeBankTable(s, d, t)
    table.insert_until(len(s))
    return table


@pytest.mark.parametrize("h", ec.hand_cases(), ids=lambda h: h["name"])
def test_hand_made_cases(h):
    empty = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    p, n = eb.edge_bank_link_prediction(_Hist(*h["history"]), h["queries"], empty, h["mode"], h["window_mode"], h["proportion"])
    assert p.tolist() == h["expected"] == ec.load_golden("hand")[f"{h['name']}|prob"].tolist()
    assert len(n) == 0 and n.dtype == np.float64
    # every mode agrees with the oracle on these histories, and a table built twice has the same bytes
    for mode, window_mode in ec.MODES:
        got = eb.edge_bank_link_prediction(_Hist(*h["history"]), h["queries"], h["queries"], mode, window_mode, h["proportion"])
        want = eo.edge_bank_link_prediction(_Hist(*h["history"]), h["queries"], h["queries"], mode, window_mode, h["proportion"])
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
    a, b = _table_of(h["history"]), _table_of(h["history"])
    assert torch.equal(a.buffer, b.buffer) and int(a.flags().item()) == 0


def test_table_state_of_the_collision_and_duplicate_cases():
    """What the table holds, read back: D, and for the colliding keys a cluster that wraps past the table's end."""
    hands = {h["name"]: h for h in ec.hand_cases()}
    t = _table_of(hands["collisions_wrap"]["history"])
    cap = eb.table_capacity(5)
    assert cap == 16 and t.buffer.numel() == 64 + 2048 + 28 * cap
    words = t.buffer[:64].view(torch.int64).cpu()
    assert int(words[0]) == 5                                                                      # distinct pairs
    keys = t.buffer[64 + 2048 + 16 * cap: 64 + 2048 + 24 * cap].view(torch.int64).cpu().numpy()
    occupied = sorted(int(i) for i in np.nonzero(keys != -1)[0])
    assert occupied == [0, 1, 2, 14, 15]                                                           # homes 14 / 15, wrapped to 0, 1, 2
    want = sorted((s << 32) | d for s, d in ec.colliding_pairs()[:5])
    assert sorted(int(k) for k in keys[occupied]) == want
    t = _table_of(hands["duplicates"]["history"])
    cap = eb.table_capacity(599)
    assert int(t.buffer[:8].view(torch.int64).item()) == 2
    count = t.buffer[64 + 2048: 64 + 2048 + 4 * cap].view(torch.int32).cpu().numpy()
    assert sorted(count[count != 0].tolist()) == [299, 300]
    first = t.buffer[64 + 2048 + 24 * cap: 64 + 2048 + 28 * cap].view(torch.int32).cpu().numpy()
    last = t.buffer[64 + 2048 + 4 * cap: 64 + 2048 + 8 * cap].view(torch.int32).cpu().numpy()
    assert sorted(first[count != 0].tolist()) == [0, 300] and sorted(last[count != 0].tolist()) == [299, 598]


def test_empty_history():
    empty = _Hist(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0))
    pos, neg = (np.array([1, 0]), np.array([2, 0])), (np.array([3]), np.array([4]))
    for mode in ("unlimited_memory", "repeat_threshold_memory"):
        p, n = eb.edge_bank_link_prediction(empty, pos, neg, mode, "fixed_proportion", 0.15)
        assert p.tolist() == [0.0, 0.0] and n.tolist() == [0.0]
    for wm in ("fixed_proportion", "repeat_interval"):
        with pytest.raises(ValueError):
            eb.edge_bank_link_prediction(empty, pos, neg, "time_window_memory", wm, 0.15)
    # the loop on an empty train ++ val: the first batch's history is empty
    c = case("gen_sorted")
    none = ec._sub(c["full"], 0, 0)
    loader = get_idx_data_loader(list(range(c["full"].num_interactions)), batch_size=200, shuffle=False)
    sampler = NegativeEdgeSampler(c["full"].src_node_ids, c["full"].dst_node_ids, seed=1)
    with pytest.raises(ValueError, match="empty sequence"):
        eb.evaluate_edge_bank_link_prediction(none, none, loader, sampler, c["full"], edge_bank_memory_mode="time_window_memory")
    scores, _ = eb.edge_bank_scores(none, none, loader, sampler, c["full"], "unlimited_memory", "fixed_proportion", 0.15)
    assert float(scores[0][0].sum().item()) == 0.0                                                 # nothing is known before the first batch


def test_refused_inputs():
    c = case("gen_unsorted")                                     # its tail is shuffled in time
    loader, sampler = loop_inputs(c)
    with pytest.raises(ValueError, match="chronological"):
        eb.evaluate_edge_bank_link_prediction(c["train"], c["val"], loader, sampler, c["test"])
    hist = _Hist([1, 1, 3], [2, 2, 4], [0.0, 1.0, 2.0])
    pos, neg = (np.array([1]), np.array([2])), (np.array([1]), np.array([4]))
    with pytest.raises(ValueError, match=str(2 ** 31)):
        eb.edge_bank_link_prediction(_Hist([1, 2 ** 31], [2, 3], [0.0, 1.0]), pos, neg, "unlimited_memory", "fixed_proportion", 0.15)
    with pytest.raises(ValueError, match=str(2 ** 31)):
        eb.edge_bank_link_prediction(hist, pos, (np.array([1]), np.array([2 ** 31])), "unlimited_memory", "fixed_proportion", 0.15)
    assert eb.edge_bank_link_prediction(hist, pos, (np.array([1]), np.array([2 ** 31 - 1])), "unlimited_memory", "fixed_proportion", 0.15)[1].tolist() == [0.0]
    with pytest.raises(ValueError, match="bogus"):
        eb.edge_bank_link_prediction(hist, pos, neg, "bogus", "fixed_proportion", 0.15)
    c = case("gen_sorted")
    loader, sampler = loop_inputs(c)
    big = ec._sub(c["test"], 0, c["test"].num_interactions)
    big.dst_node_ids = big.dst_node_ids.copy()
    big.dst_node_ids[-1] = 2 ** 31
    with pytest.raises(ValueError, match=str(2 ** 31)):
        eb.evaluate_edge_bank_link_prediction(c["train"], c["val"], loader, sampler, big)
    # the library's own checks arrive as ValueError: a query for another H than the edges inserted
    table = eb.EdgeBankTable(*[np.asarray(x) for x in ([1, 1, 3], [2, 2, 4], [0.0, 1.0, 2.0])])
    table.insert_until(2)
    q = torch.tensor([1], device="cuda")
    rc = table.lib.dygnn_edgebank_query(table.c, table.times.data_ptr(), 0, 0, 3, 0.0, q.data_ptr(), q.data_ptr(), 1,
                                        torch.empty(1, device="cuda").data_ptr(), None)
    with pytest.raises(ValueError, match="exceeds the 2 edges inserted"):
        _capi.check(rc, ValueError)


def test_kernels_guard_ids_the_host_checks_would_refuse():
    """Past the Python checks, straight into the library: ids outside [0, 2^31) are neither hashed nor stored; the guard word says so."""
    src = np.array([1, 2 ** 31, -1, 5, 2 ** 40], dtype=np.int64)
    dst = np.array([2, 3, 4, -(2 ** 31), 6], dtype=np.int64)
    table = eb.EdgeBankTable(src, dst, np.arange(5.0))
    table.insert_until(5)
    assert int(table.buffer[:8].view(torch.int64).item()) == 1                                     # only (1, 2) was stored
    for mode, window_mode in ((0, 0), (1, 0), (2, 0), (2, 1)):
        out = table.query(mode, window_mode, 0.0, torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda())
        # H counts all five positions, so the one stored pair (count 1) is below the threshold 5 / 1
        assert out.tolist() == [0.0 if mode == 1 else 1.0, 0.0, 0.0, 0.0, 0.0]
    assert int(table.flags().item()) == 1
    with pytest.raises(_capi.DygnnError, match="outside"):
        eb._raise_on_flags(int(table.flags().item()))


def test_layout_is_a_function_of_the_key_set_not_of_the_order():
    """Ordered probing: one insert of the same edges in another order leaves the same keys in the same slots with the same counts and
    latest times (only the positions differ).  3000 edges over 200 x 200 pairs are nearly all distinct: load ~0.35 of the 8192 slots, so
    probe clusters of several keys are common."""
    from dyglib_amd import synthetic as syn
    d, _, _ = syn.make_general_graph(200, 3000, seed=8)
    src, dst, t = d.src_node_ids, d.dst_node_ids, d.node_interact_times
    cap = eb.table_capacity(3000)
    lo = 64 + 2048

    def arrays(order):
        table = _table_of((src[order], dst[order], t[order]))
        assert int(table.flags().item()) == 0
        b = table.buffer
        return (b[:16].clone(), b[lo: lo + 4 * cap].clone(), b[lo + 8 * cap: lo + 24 * cap].clone())      # D and end; count; max_time and keys

    base = arrays(np.arange(3000))
    n_pairs = len(set(zip(src.tolist(), dst.tolist())))
    assert int(base[0][:8].view(torch.int64).item()) == n_pairs > 2800
    homes = np.array([eb.home_slot(a, b, cap) for a, b in set(zip(src.tolist(), dst.tolist()))])
    assert len(np.unique(homes)) < n_pairs - 300                                     # hundreds of keys do not get their home slot
    for seed in (0, 1):
        other = arrays(np.random.RandomState(seed).permutation(3000))
        assert all(torch.equal(x, y) for x, y in zip(base, other))
    # ... and two ranges give the keys of earlier ranges their slots for good: the first range's layout survives the second
    table = eb.EdgeBankTable(src, dst, t)
    table.insert_until(1500)
    keys_a = table.buffer[lo + 16 * cap: lo + 24 * cap].view(torch.int64).clone()
    table.insert_until(3000)
    keys_b = table.buffer[lo + 16 * cap: lo + 24 * cap].view(torch.int64)
    held = keys_a != -1
    assert torch.equal(keys_a[held], keys_b[held]) and int((keys_b != -1).sum().item()) == n_pairs


def test_larger_graph_against_the_oracle_across_workgroups():
    """6000 edges over 35 x 20 node pairs (many repeats, long probe clusters), 1000 in the table before the first batch and 500 more per
    batch (two workgroups per insert), every mode, against the CPU oracle's per-batch rebuild."""
    from dyglib_amd import synthetic as syn
    d, _, _ = syn.make_bipartite_graph(35, 20, 6000, seed=3)
    src, dst, t = d.src_node_ids, d.dst_node_ids, d.node_interact_times
    base, B = 1000, 500
    batches = [np.arange(a, a + B) for a in range(0, 6000 - base, 1000)]                        # every other 500: inserts of 1000 between queries
    rs = np.random.RandomState(4)
    negs = [(src[base + i], rs.choice(np.unique(dst), B)) for i in batches]
    for mode, window_mode in ec.MODES:
        want = eo.evaluate(src, dst, t, base, batches, negs, mode, window_mode, ec.TEST_RATIO)
        if mode == "time_window_memory":                                                          # the margin condition, on the oracle's start
            for i in batches:
                h = base + int(i[0])
                start = eo.window_start(src[:h], dst[:h], t[:h], window_mode, ec.TEST_RATIO)
                assert np.abs(t[:h] - start).min() / (t[:h].max() - t[:h].min()) >= ec.MARGIN
        m, wm = eb._modes(mode, window_mode)
        table = eb.EdgeBankTable(src, dst, t)
        q_src = torch.from_numpy(np.stack([np.concatenate([src[base + i], n[0]]) for i, n in zip(batches, negs)])).cuda()
        q_dst = torch.from_numpy(np.stack([np.concatenate([dst[base + i], n[1]]) for i, n in zip(batches, negs)])).cuda()
        hist = np.array([base + int(i[0]) for i in batches])
        starts = torch.tensor([eb.window_start_time(t[:h], ec.TEST_RATIO) for h in hist], dtype=torch.float64).cuda() if (m, wm) == (2, 0) else None
        got = table.evaluate(hist, starts, q_src, q_dst, m, wm).cpu().numpy()
        np.testing.assert_array_equal(got.astype(np.float64), np.stack(want))
        assert 0 < got.mean() < 1 and int(table.flags().item()) == 0
