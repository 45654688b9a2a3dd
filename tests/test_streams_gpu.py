"""Every backbone and device primitive on a stream that is not the default one, one model on two streams at once, and DyGFormer's caches handed
from the stream that builds them to another (tests/stream_cases.py holds the helpers and the case list).

a. Wrong-stream detection.  The call's device inputs hold ANOTHER valid batch; on a side stream, behind a blocker, the real batch is copied in
   and the call is made.  A kernel, fill or copy the library issued on any other stream has by then run against the other batch, or against a
   workspace nothing has written, and the result differs.  Expected: the same call on the default stream, itself held to the reference fixture or
   oracle at the backbone's own bar -- bit for bit for everything the suite already holds to run-to-run bit equality; gradients (atomic sums)
   against the oracle at the scaled gradient bar on both streams.
b. Two concurrent streams issue interleaved calls of ONE model on different batches (what bench.py --streams 2 does): every result equals the
   serial default-stream result bit for bit.  Overlap is not forced; the test can fail only for a fault in the per-stream workspaces.
c. DyGFormer's kernel-ready weights and projected feature tables are built by launches alone, on the stream of the call that finds them stale.
   A call on stream B, issued while the build is still held up on stream A, must wait for it.  What makes a too-short hold visible is the
   assertion that B's call was ISSUED while A was still held: once the library orders the hand-off, B can no longer FINISH while A is held
   (it waits for the build), so that form of the assertion holds only for the unordered code -- where it was observed, with B's embeddings
   0.08 .. 0.16 away from the oracle.  That the two streams do run concurrently is established by the `pair` fixture.

Hold lengths are not fixed: ten times the measured host time of enqueueing what has to land behind the hold, at least 20 ms, at most 250 ms;
every test prints what it measured and asserts that the hold was still in place when the enqueue had finished."""
import numpy as np
import pytest
import torch

from dyglib_amd import synthetic as syn
from oracle import dygformer_oracle as orc
from tests import golden_cases as gc
from tests import stream_cases as sc
from tests.parity import close

pytestmark = pytest.mark.gpu
DEV = sc.DEV
K_INTERLEAVED = 8


@pytest.fixture(scope="module")
def pair():
    return sc.concurrent_pair(DEV)


def _on_device(arrays):
    out = {k: sc._dev(v) for k, v in arrays.items()}
    torch.cuda.synchronize()
    return out


# ---- a. every entry on a side stream ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.CASES, ids=sc.CASE_NAMES)
def test_side_stream_call_equals_default_stream_call(case):
    case.setup()
    real = _on_device(case.inputs())
    # the default stream, held to the reference
    case.reset()
    base_bits, base_extra = case.call(real)
    torch.cuda.synchronize()
    case.check(base_bits, base_extra, "default stream")
    # one warm run of exactly what will be issued behind the hold: its host time sizes the hold
    bufs = _on_device(case.stale())
    case.reset()
    torch.cuda.synchronize()

    def enqueue():
        for k in bufs:
            bufs[k].copy_(real[k], non_blocking=True)
        case.call(bufs)
    enqueue_ms = sc.timed_ms(enqueue)
    torch.cuda.synchronize()
    hold = sc.hold_ms(enqueue_ms)
    # the side stream: the inputs hold the other batch until the copies behind the blocker have run
    for k, v in _on_device(case.stale()).items():
        bufs[k].copy_(v)
    case.reset()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    with sc.no_collector_pauses(), torch.cuda.stream(side):
        ev = sc.blocker(side, hold)
        for k in bufs:
            bufs[k].copy_(real[k], non_blocking=True)
        held_after_copies = not ev.query()
        bits, extra = case.call(bufs, lambda: sc.blocker(side, hold))
        held_after_call = not ev.query()
    side.synchronize()
    print(f"streams {case.name}: enqueue {enqueue_ms:.2f} ms, hold {hold:.0f} ms, held after the copies: {held_after_copies}, after the call: {held_after_call}")
    assert held_after_copies, f"the {hold:.0f} ms hold ended before the input copies were enqueued (enqueue measured {enqueue_ms:.2f} ms)"
    if case.returns_without_waiting:
        assert held_after_call, f"the {hold:.0f} ms hold ended before the call was enqueued (enqueue measured {enqueue_ms:.2f} ms)"
    assert len(bits) == len(base_bits)
    for i, (a, b) in enumerate(zip(base_bits, bits)):
        assert torch.equal(a, b), f"{case.name}: output {i} on the side stream differs from the default stream's (max |diff| {float((a.double() - b.double()).abs().max()):.3e})"
    case.check(bits, extra, "side stream")


# ---- b. one model, two streams, different batches ----------------------------------------------------------------------------------------------
def _batches(c, k, n):
    """k different batches of n interactions of the case's graph, with negative destinations"""
    d = c["data"]
    E = d.num_interactions
    uniq = np.unique(d.dst_node_ids)
    out = []
    for j in range(k):
        idx = (np.arange(n) * 7 + 13 * j + E // 2) % E
        out.append(dict(src=d.src_node_ids[idx].astype(np.int64), dst=d.dst_node_ids[idx].astype(np.int64), times=d.node_interact_times[idx].astype(np.float64),
                        neg=syn.random_negative_dst(np.random.RandomState(j), uniq, n).astype(np.int64)))
    return out


def _interleaved_equals_serial(pair, batches, call):
    dev_batches = [_on_device(b) for b in batches]
    with torch.no_grad():
        serial = [call(b) for b in dev_batches]
        torch.cuda.synchronize()
        outs = []
        for j, b in enumerate(dev_batches):
            with torch.cuda.stream(pair[j % 2]):
                outs.append(call(b))
    pair[0].synchronize()
    pair[1].synchronize()
    assert not all(torch.equal(serial[0][0], s[0]) for s in serial[1:])          # the batches differ
    for j, (want, got) in enumerate(zip(serial, outs)):
        for a, b in zip(want, got):
            assert torch.equal(a, b), f"call {j} (stream {j % 2})"


def test_dygformer_many_on_two_streams_equals_serial(pair):
    from tests.test_dygformer_gpu import build_model
    c = gc.build_case("gen_p1_l32")
    model, _ = build_model(c)

    def call(b):
        s, d = model.compute_src_dst_node_temporal_embeddings_many(torch.stack([b["src"], b["src"]]), torch.stack([b["dst"], b["neg"]]),
                                                                   torch.stack([b["times"], b["times"]]), pos_neg_halves=True)
        return s, d
    _interleaved_equals_serial(pair, _batches(c, K_INTERLEAVED, 24), call)


def test_tgat_on_two_streams_equals_serial(pair):
    from tests.test_tgat import _model
    c = gc.build_tgat_case("tgat_gen_l2_k5")
    model = _model(c)
    k = c["tgat_cfg"]["num_neighbors"]
    _interleaved_equals_serial(pair, _batches(c, K_INTERLEAVED, 24),
                               lambda b: model.compute_src_dst_node_temporal_embeddings(b["src"], b["dst"], b["times"], num_neighbors=k))


# ---- c. DyGFormer: caches built on one stream, read on another ---------------------------------------------------------------------------------
class _Fresh:
    """A DyGFormer nothing else in the process shares weights or tables with (the caching allocator may hand a new model the block that held an
    earlier model's tables: with unique values a table that was never built cannot pass for a built one), its oracle, and a small batch."""
    P, L, N = 1, 32, 12

    def __init__(self, seed):
        from dyglib_amd import DyGFormer, get_neighbor_sampler
        c = gc.build_case("gen_p1_l32")
        d = c["data"]
        rs = np.random.RandomState(seed)
        self.nf = (0.5 * rs.standard_normal(c["node_feat"].shape)).astype(np.float32)
        self.nf[0] = 0.0
        self.ef = (0.5 * rs.standard_normal(c["edge_feat"].shape)).astype(np.float32)
        self.ef[0] = 0.0
        self.params = syn.make_dygformer_params(seed, patch_size=self.P)
        self.adj = orc.OracleAdjacency(d.src_node_ids, d.dst_node_ids, d.edge_ids, d.node_interact_times)
        self.batch = [dict(src=c["src"][sl], dst=c["dst"][sl], times=c["times"][sl]) for sl in (slice(0, self.N), slice(self.N, 2 * self.N))]
        sampler = get_neighbor_sampler(d, "recent", seed=1, device=DEV)
        m = DyGFormer(self.nf, self.ef, sampler, 100, 50, patch_size=self.P, num_layers=2, num_heads=2, dropout=0.1, max_input_sequence_length=self.L, device=DEV)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in self.params.items()}, strict=True)
        self.model = m.to(DEV).eval()
        self.model._fixed_dropout_seed = 77
        self.dev_batch = [_on_device(b) for b in self.batch]

    def oracle(self, i):
        b = self.batch[i]
        with torch.no_grad():
            s, d = orc.dygformer_forward(self.params, self.nf, self.ef, self.adj, b["src"], b["dst"], b["times"], self.P, self.L)
        return s.numpy(), d.numpy()

    def infer(self, i):
        b = self.dev_batch[i]
        with torch.no_grad():
            return self.model.compute_src_dst_node_temporal_embeddings(b["src"], b["dst"], b["times"])

    def train_forward(self, i):
        b = self.dev_batch[i]
        return self.model.compute_src_dst_node_temporal_embeddings(b["src"], b["dst"], b["times"])

    def update(self, step):
        """an in-place weight update (what an optimizer step is), on the current stream; the host copy follows with the same float32 operations"""
        scale, shift = np.float32(1.0 + 0.25 * step), np.float32(0.25 * step)
        with torch.no_grad():
            self.model.projection_layer["edge"].weight.mul_(float(scale))
            self.model.output_layer.bias.add_(float(shift))
        self.params = dict(self.params)
        self.params["projection_layer.edge.weight"] = self.params["projection_layer.edge.weight"] * scale
        self.params["output_layer.bias"] = self.params["output_layer.bias"] + shift

    def check(self, got, i, what):
        ws, wd = self.oracle(i)
        close(sc._np(got[0]), ws, f"{what}: src emb", label="streams: dygformer cache hand-off vs oracle")
        close(sc._np(got[1]), wd, f"{what}: dst emb", label="streams: dygformer cache hand-off vs oracle")

    def params_match_the_model(self):
        sd = self.model.state_dict()
        return all(np.array_equal(sc._np(sd[k]), v) for k, v in self.params.items())


def _hand_off(pair, what, enqueue_ms, on_a, on_b):
    """Hold A; issue on_a() under A (it queues the cache's build behind the hold) and on_b() under B.  B's call must have been issued while the
    hold was still in place -- with `pair` running concurrently, nothing but the library's own ordering then keeps B from running ahead of
    the build.  Returns (A's result, B's result) after both streams have finished."""
    a, b = pair
    hold = sc.hold_ms(enqueue_ms)
    torch.cuda.synchronize()
    with sc.no_collector_pauses():
        ev = sc.blocker(a, hold)
        with torch.cuda.stream(a):
            out_a = on_a()
        with torch.cuda.stream(b):
            out_b = on_b()
        issued_behind_the_hold = not ev.query()
    b.synchronize()
    ran_ahead = not ev.query()
    a.synchronize()
    print(f"streams {what}: enqueue {enqueue_ms:.2f} ms, hold {hold:.0f} ms, B issued while A was held: {issued_behind_the_hold}, "
          f"B finished while A was held: {ran_ahead}")
    assert issued_behind_the_hold, f"{what}: the {hold:.0f} ms hold ended before both calls were enqueued (enqueue measured {enqueue_ms:.2f} ms)"
    return out_a, out_b


@pytest.fixture
def tables(monkeypatch):
    monkeypatch.setenv("DYGNN_PROJ_TABLES", "1")
    monkeypatch.delenv("DYGNN_POOLED_TAIL", raising=False)
    return monkeypatch


def test_projected_tables_built_on_one_stream_are_ready_on_another(pair, tables):
    """c1: the first inference call after a pack builds the tables on ITS stream; a call on another stream reads them"""
    def prepared(seed):
        f = _Fresh(seed)
        tables.setenv("DYGNN_PROJ_TABLES", "0")
        f.infer(0)                                   # the full pack (it synchronises its stream); no tables yet
        tables.setenv("DYGNN_PROJ_TABLES", "1")
        torch.cuda.synchronize()
        assert f.model._tables.built == set()
        return f
    twin = prepared(9101)                            # the same sequence once without a hold, on a twin: its host time sizes the hold
    a, b = pair

    def sequence(f):
        with torch.cuda.stream(a):
            f.infer(0)
        with torch.cuda.stream(b):
            f.infer(1)
    enqueue_ms = sc.timed_ms(lambda: sequence(twin))
    torch.cuda.synchronize()
    f = prepared(9102)
    out_a, out_b = _hand_off(pair, "c1 projected tables", enqueue_ms, lambda: f.infer(0), lambda: f.infer(1))
    assert f.model._tables.built == {"node", "edge"}
    f.check(out_b, 1, "c1: call on B while the tables' build was held on A")
    f.check(out_a, 0, "c1: the building call on A")


@pytest.mark.parametrize("training_forward_first", [False, True], ids=["c2_repack", "c3_packed_complete"])
def test_weights_repacked_on_one_stream_are_ready_on_another(pair, tables, training_forward_first):
    """c2: after an in-place weight update the next call refreshes the kernel-ready copy with launches alone, on its stream.  c3: a training
    forward (here: eval mode with autograd recording, so that no train() / eval() switch drops the copy) refreshes the training sections only;
    the next inference call brings the inference sections up to date, again with launches alone.
    The caller orders B after its own weight write (wait_stream); the refresh is the library's."""
    f = _Fresh(9200 + int(training_forward_first))
    a, b = pair
    def sequence(step, held):
        with torch.cuda.stream(a):
            f.update(step)
            if training_forward_first:
                f.train_forward(0)
        b.wait_stream(a)
        if held:
            return _hand_off(pair, "c3 packed-complete branch" if training_forward_first else "c2 repack", held, lambda: f.infer(0), lambda: f.infer(1))
        with torch.cuda.stream(a):
            f.infer(0)
        with torch.cuda.stream(b):
            f.infer(1)

    with torch.cuda.stream(a):
        f.infer(0)                                   # warm on A: the kernel-ready copy and the tables exist
    torch.cuda.synchronize()
    before = f.oracle(1)
    enqueue_ms = sc.timed_ms(lambda: sequence(1, None))          # a first update, unheld: the host time of the sequence
    torch.cuda.synchronize()
    out_a, out_b = sequence(2, enqueue_ms)
    after = f.oracle(1)
    assert all(float(np.abs(x - y).max()) > 100 * 1e-4 for x, y in zip(before, after))          # the updates move the embeddings far beyond the bar
    assert f.params_match_the_model()
    f.check(out_b, 1, "call on B while the refresh was held on A")
    f.check(out_a, 0, "the refreshing call on A")
