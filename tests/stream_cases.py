"""Helpers and the case list of the stream tests (tests/test_streams_gpu.py, tests/test_streams_cpu.py).  Importable without a GPU.

Every public backbone and device primitive has one case here, at the smallest recipe of its own case module.  A case knows
  inputs()   the real batch, name -> ndarray, exactly the arrays the call reads from the device;
  stale()    another VALID batch of the same shapes (every array rolled by its own shift: ids stay ids of the graph, times stay times), so
             that a launch which reads the inputs too early computes a wrong answer and never an out-of-range address;
  setup()    the model on the GPU, its references loaded;
  call(t)    one call on device tensors `t` (same keys as inputs()) under the CURRENT stream -> (bits, extra): `bits` are the outputs the
             existing suite already holds to run-to-run bit equality (inference rows, seeded-dropout forward rows, state the call leaves),
             `extra` whatever is compared with a reference at a tolerance only (gradients: atomic sums);
  check()    holds (bits, extra) to the reference fixture / oracle at the bar the backbone's own GPU test uses;
  reset()    puts back the state a call changed (memory bank from a backup, gradients to None).

The blocker holds a stream for a measured number of milliseconds without occupying the chip (torch.cuda._sleep spins one thread); the
cycles-to-milliseconds ratio is measured once per process, never assumed."""
from __future__ import annotations

import contextlib
import functools
import gc as gc_module
import time

import numpy as np

from tests import golden_cases as gc

DEV = "cuda:0"
MAX_HOLD_MS = 250.0          # no single hold is longer
MIN_HOLD_MS = 20.0
HOLD_FACTOR = 10.0           # hold = HOLD_FACTOR x the measured host enqueue time (host jitter on a shared machine)
MAX_STREAMS = 8

# names dyglib_amd exports that launch nothing of their own: host code, or loops over the calls the cases below cover
HOST_ONLY = {
    "InteractionData": "host container", "Data": "host container", "get_link_prediction_data": "reads dataset files on the host",
    "NegativeEdgeSampler": "host numpy sampler", "get_idx_data_loader": "host index loader",
    "compute_src_dst_node_time_shifts": "host numpy statistics", "TimeEncoder": "parameters only: evaluated inside the backbones' kernels",
    "TemporalCSR": "host builder; its one upload is a blocking copy (dyglib_amd/temporal_csr.py: on_device)",
    "evaluate_model_link_prediction": "host loop over a backbone call, MergeLayer and the metrics kernel",
    "evaluate_memory_model_link_prediction": "host loop over a memory model's step, MergeLayer and the metrics kernel",
    "evaluate_edge_bank_link_prediction": "host loop over EdgeBankTable and the metrics kernel",
}


# ---- the blocker -------------------------------------------------------------------------------------------------------------------------------
_CYCLES_PER_MS = {}


def cycles_per_ms(dev=DEV) -> float:
    """torch.cuda._sleep cycles per millisecond on `dev`, from one short hold timed with events (grown tenfold, three times at the most,
    until the hold lasts a millisecond: the counter's rate is not assumed).  The sleep kernel runs once untimed first -- a process's first
    launch of it includes loading it, about a millisecond that is no hold -- and the accepted hold is timed a second time: the two must agree."""
    import torch
    if dev not in _CYCLES_PER_MS:
        s = torch.cuda.Stream(dev)

        def timed(cycles):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                e0.record()
                torch.cuda._sleep(cycles)
                e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        timed(1000)
        cycles, ms = 100_000, 0.0
        for _ in range(4):
            ms = timed(cycles)
            if ms >= 1.0:
                break
            cycles *= 10
        again = timed(cycles)
        assert 1.0 <= ms <= MAX_HOLD_MS and abs(again - ms) <= 0.2 * ms, f"calibration holds of {cycles} cycles took {ms} ms and {again} ms"
        _CYCLES_PER_MS[dev] = cycles / ms
    return _CYCLES_PER_MS[dev]


def hold_ms(enqueue_ms: float) -> float:
    """the hold that covers calls whose host enqueue took `enqueue_ms`"""
    return min(MAX_HOLD_MS, max(MIN_HOLD_MS, HOLD_FACTOR * enqueue_ms))


def blocker(stream, ms: float):
    """Keep `stream` busy for about `ms` milliseconds (at most MAX_HOLD_MS); returns an event recorded behind the hold."""
    import torch
    ms = min(float(ms), MAX_HOLD_MS)
    ev = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(ms * cycles_per_ms(str(stream.device))))
        ev.record(stream)
    return ev


@contextlib.contextmanager
def no_collector_pauses():
    """Python's cyclic garbage collector switched off while calls are enqueued behind a hold: late in a long test run one of its full passes
    takes longer than a whole hold.  (Collected once before, switched back on afterwards; reference counting frees everything as usual.)"""
    gc_module.collect()
    was_enabled = gc_module.isenabled()
    gc_module.disable()
    try:
        yield
    finally:
        if was_enabled:
            gc_module.enable()


def timed_ms(fn) -> float:
    """wall clock around fn() in milliseconds: the host time to enqueue what fn issues"""
    with no_collector_pauses():
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3


def concurrent_pair(dev=DEV):
    """Two streams of at most MAX_STREAMS that demonstrably run concurrently: while the first is held, a trivial kernel on the second runs to
    completion.  A bounded selection among fresh streams, not a retry; AssertionError when no pair qualifies (every process here gets
    several hardware queues, so none qualifying is a finding, not a reason to skip)."""
    import torch
    streams = [torch.cuda.Stream(dev) for _ in range(MAX_STREAMS)]
    torch.cuda.synchronize()
    a = streams[0]
    for b in streams[1:]:
        ev = blocker(a, MIN_HOLD_MS)
        with torch.cuda.stream(b):
            x = torch.zeros(64, device=dev) + 1.0
        b.synchronize()
        ran_ahead = not ev.query()
        a.synchronize()
        assert float(x.sum()) == 64.0
        if ran_ahead:
            return a, b
    raise AssertionError(f"no two of {MAX_STREAMS} streams ran concurrently: a {MIN_HOLD_MS} ms hold on one stream delayed a kernel on every other")


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
def _dev(x, dev=DEV):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _load(model, params):
    import torch
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return model


class StreamCase:
    name = ""
    covers = ()                            # names of dyglib_amd.__all__ this case runs
    roll_axis = 0
    returns_without_waiting = False        # read from the call's code: it ends without a host synchronisation (the hold outlives the enqueue)

    def inputs(self) -> dict:
        raise NotImplementedError

    def stale(self) -> dict:
        return {k: np.ascontiguousarray(np.roll(v, i + 1, axis=self.roll_axis)) for i, (k, v) in enumerate(self.inputs().items())}

    def setup(self) -> None:
        raise NotImplementedError

    def reset(self) -> None:
        pass

    def call(self, t: dict, hold=None):
        raise NotImplementedError

    def check(self, bits, extra, tag: str) -> None:
        raise NotImplementedError


class _PairCase(StreamCase):
    """a backbone's pair call on (src, dst, times) of its recipe, against the reference fixture's src_emb / dst_emb"""
    golden = ""
    keys = ("src_emb", "dst_emb")

    def inputs(self):
        c = self.c
        return dict(src=c["src"].astype(np.int64), dst=c["dst"].astype(np.int64), times=c["times"].astype(np.float64))

    def check(self, bits, extra, tag):
        from tests.parity import close
        g = gc.load_golden(self.golden)
        for got, key in zip(bits, self.keys):
            close(_np(got), g[key], f"{self.name} {tag} {key}", label=f"streams: {self.name} vs reference")


class DygformerInference(_PairCase):
    covers = ("DyGFormer",)
    returns_without_waiting = True         # device inputs, weights packed and CSR uploaded by the first call: launches only

    def __init__(self, impl):
        self.impl = impl
        self.name = "dygformer_impl%d" % impl
        self.golden = "gen_p1_l32"

    @functools.cached_property
    def c(self):
        return gc.build_case("gen_p1_l32")

    def setup(self):
        from tests.test_dygformer_gpu import build_model
        self.model, _ = build_model(self.c)
        self.model.impl = self.impl

    def call(self, t, hold=None):
        import torch
        with torch.no_grad():
            return list(self.model.compute_src_dst_node_temporal_embeddings(t["src"], t["dst"], t["times"])), {}


class DygformerMany(StreamCase):
    """[positive call ; negative call] in one launch, the two pairs of an edge in one workgroup"""
    name = "dygformer_many_pos_neg_halves"
    covers = ("DyGFormer",)
    roll_axis = 1
    returns_without_waiting = True

    def inputs(self):
        c = gc.build_case("gen_p1_l32")
        return dict(src=np.stack([c["src"], c["src"]]).astype(np.int64), dst=np.stack([c["dst"], c["neg_dst"]]).astype(np.int64),
                    times=np.stack([c["times"], c["times"]]).astype(np.float64))

    def setup(self):
        from tests.test_dygformer_gpu import build_model
        self.model, _ = build_model(gc.build_case("gen_p1_l32"))

    def call(self, t, hold=None):
        import torch
        with torch.no_grad():
            s, d = self.model.compute_src_dst_node_temporal_embeddings_many(t["src"], t["dst"], t["times"], pos_neg_halves=True)
        return [s[0], d[0], s[1], d[1]], {}

    def check(self, bits, extra, tag):
        from tests.parity import close
        g = gc.load_golden("gen_p1_l32")
        for got, key in zip(bits, ("src_emb", "dst_emb", "neg_src_emb", "neg_dst_emb")):
            close(_np(got), g[key], f"{self.name} {tag} {key}", label="streams: dygformer many vs reference")


class TgatInference(_PairCase):
    name, covers, golden = "tgat", ("TGAT",), "tgat_hub_l1_k10"

    @functools.cached_property
    def c(self):
        return gc.build_tgat_case("tgat_hub_l1_k10")

    def setup(self):
        from tests.test_tgat import _model
        self.model = _model(self.c)

    def call(self, t, hold=None):
        import torch
        with torch.no_grad():
            return list(self.model.compute_src_dst_node_temporal_embeddings(t["src"], t["dst"], t["times"], num_neighbors=self.c["tgat_cfg"]["num_neighbors"])), {}


class TclInference(_PairCase):
    name, covers, golden = "tcl", ("TCL",), "tcl_gen_k5_l1_h2"

    @functools.cached_property
    def c(self):
        from tests import tcl_cases as tc
        return tc.build_tcl_case("gen_k5_l1_h2")

    def setup(self):
        from tests.test_tcl_gpu import case_model
        _, self.cfg, self.model = case_model("gen_k5_l1_h2")

    def call(self, t, hold=None):
        import torch
        with torch.no_grad():
            return list(self.model.compute_src_dst_node_temporal_embeddings(t["src"], t["dst"], t["times"], num_neighbors=self.cfg["K"])), {}


class CawnInference(_PairCase):
    name, covers, golden = "cawn", ("CAWN",), "cawn_gen_w1_k5"

    @functools.cached_property
    def c(self):
        from tests import cawn_cases as cc
        return cc.build_cawn_case("gen_w1_k5")

    def setup(self):
        import torch
        from dyglib_amd import CAWN, get_neighbor_sampler
        from tests import cawn_cases as cc
        c = self.c
        self.cfg = cfg = c["cawn_cfg"]
        sampler = get_neighbor_sampler(c["data"], cfg["strategy"], time_scaling_factor=cfg["scale"], seed=cfg["sampler_seed"], device=DEV)
        m = CAWN(c["node_feat"], c["edge_feat"], sampler, cc.TIME_FEAT_DIM, cfg["P"], walk_length=cfg["W"], num_walk_heads=cfg["heads"], dropout=0.1, device=DEV)
        self.model = _load(m, c["cawn_params"]).to(DEV).eval()

    def call(self, t, hold=None):
        import torch
        with torch.no_grad():
            return list(self.model.compute_src_dst_node_temporal_embeddings(t["src"], t["dst"], t["times"], num_neighbors=self.cfg["k"])), {}


class GraphMixerInference(_PairCase):
    name, covers, golden = "graphmixer", ("GraphMixer",), "graphmixer_gen_k10_g7"

    @functools.cached_property
    def c(self):
        from tests import graphmixer_cases as gmc
        return gmc.build_graphmixer_case("gen_k10_g7")

    def setup(self):
        from tests.test_graphmixer_gpu import case_model
        _, self.cfg, self.model = case_model("gen_k10_g7")

    def call(self, t, hold=None):
        import torch
        with torch.no_grad():
            return list(self.model.compute_src_dst_node_temporal_embeddings(t["src"], t["dst"], t["times"], num_neighbors=self.cfg["K"],
                                                                            time_gap=self.cfg["G"])), {}


class _MemoryStep(StreamCase):
    """The LAST batch of a chronological run as one step (negative call and positive call in one library call), the memory update included: the
    batches before it are replayed on the default stream, the bank is backed up, and every run of the step starts from that backup.  Rows and
    the bank left behind against the reference fixture."""
    golden = ""
    k = 20

    def batches(self):
        raise NotImplementedError

    def build(self):
        raise NotImplementedError

    def inputs(self):
        b = self.batches()[-1]
        return dict(src=b["src"].astype(np.int64), dst=b["dst"].astype(np.int64), neg=b["neg"].astype(np.int64), t=b["t"].astype(np.float64),
                    eid=b["eid"].astype(np.int64))

    def setup(self):
        import torch
        self.model = self.build()
        with torch.no_grad():
            for b in self.batches()[:-1]:
                self.model.compute_step_embeddings(b["src"], b["dst"], b["src"], b["neg"], b["t"], b["eid"], num_neighbors=self.k)
        torch.cuda.synchronize()
        self.backup = self.model.memory_bank.backup_memory_bank()

    def reset(self):
        self.model.memory_bank.reload_memory_bank(self.backup)

    def bank(self):
        mb = self.model.memory_bank
        return [x.clone() for x in (mb.node_memories.data, mb.node_last_updated_times.data, mb.msg, mb.msg_time, mb.has_msg)]

    def call(self, t, hold=None):
        import torch
        with torch.no_grad():
            rows = self.model.compute_step_embeddings(t["src"], t["dst"], t["src"], t["neg"], t["t"], t["eid"], num_neighbors=self.k)
            return list(rows) + self.bank(), {}

    def check(self, bits, extra, tag):
        from tests.parity import close
        g = gc.load_golden(self.golden)
        i = len(self.batches()) - 1
        for got, key in zip(bits[:4], ("pos_src", "pos_dst", "neg_src", "neg_dst")):
            close(_np(got), g[f"b{i}_{key}"], f"{self.name} {tag} batch {i} {key}", label=f"streams: {self.name} vs reference")
        close(_np(bits[4]), g["final_memory"], f"{self.name} {tag} memory", label=f"streams: {self.name} vs reference")
        close(_np(bits[5]), g["final_last_update"], f"{self.name} {tag} last update", label=f"streams: {self.name} vs reference")


class TgnStep(_MemoryStep):
    name, covers, golden = "tgn_step", ("MemoryModel",), "tgn_gen_l2_k4"

    def batches(self):
        return gc.build_tgn_case("tgn_gen_l2_k4")["tgn_batches"]

    def build(self):
        from tests.test_tgn_train_gpu import _model
        c = gc.build_tgn_case("tgn_gen_l2_k4")
        self.k = c["tgn_cfg"]["num_neighbors"]
        return _model(c, train=False)


class JodieStep(_MemoryStep):
    name, covers, golden = "jodie_step", ("JODIE",), "jodie_gen"

    def batches(self):
        from tests import memory_variant_cases as mv
        return mv.build_case("jodie_gen")["batches"]

    def build(self):
        from tests import memory_variant_cases as mv
        from tests.test_memory_variants_gpu import _case_model
        return _case_model(mv.build_case("jodie_gen"))


class DyrepStep(_MemoryStep):
    name, covers, golden = "dyrep_step", ("DyRep",), "dyrep_gen"

    def batches(self):
        from tests import memory_variant_cases as mv
        return mv.build_dyrep_case("dyrep_gen")["batches"]

    def build(self):
        from tests import memory_variant_cases as mv
        from tests.test_memory_variants_gpu import _dyrep
        c = mv.build_dyrep_case("dyrep_gen")
        self.k = c["cfg"]["num_neighbors"]
        return _dyrep(c)[0]


class EdgeBankCase(StreamCase):
    """table reset, insert of the history and one query of [positives ; negatives]: the first batch of the smallest loop recipe, in the mode that
    reads counts AND times (time window, fixed proportion); scores exactly as the reference's"""
    name = "edgebank_update_and_query"
    covers = ("edge_bank_link_prediction",)
    returns_without_waiting = True
    case, key = "gen_sorted", "window_fixed"

    def inputs(self):
        from tests import edgebank_cases as ec
        c, g = ec.build_case(self.case), ec.load_golden(self.case)
        h, idx = ec.history_of(c, 0), c["batches"][0]
        src = c["test"].src_node_ids[idx]
        return dict(h_src=h.src_node_ids.astype(np.int64), h_dst=h.dst_node_ids.astype(np.int64), h_t=h.node_interact_times.astype(np.float64),
                    q_src=np.concatenate([src, src]).astype(np.int64),
                    q_dst=np.concatenate([c["test"].dst_node_ids[idx], g["neg_dst"][:len(idx)]]).astype(np.int64))

    def setup(self):
        from dyglib_amd import edgebank as eb
        from tests import edgebank_cases as ec
        x = self.inputs()
        self.table = eb.EdgeBankTable(x["h_src"], x["h_dst"], x["h_t"])
        self.modes = eb._modes(*dict(zip(ec.MODE_KEYS, ec.MODES))[self.key])
        self.start = eb.window_start_time(x["h_t"], ec.TEST_RATIO)
        self.want = ec.load_golden(self.case)[f"{self.key}|prob"][:len(x["q_src"])]

    def call(self, t, hold=None):
        tb = self.table
        tb.src, tb.dst, tb.times = t["h_src"], t["h_dst"], t["h_t"]
        tb.reset()
        tb.insert_until(len(t["h_src"]))
        return [tb.query(self.modes[0], self.modes[1], self.start, t["q_src"], t["q_dst"]), tb.flags().clone()], {}

    def check(self, bits, extra, tag):
        assert int(bits[1].item()) == 0
        np.testing.assert_array_equal(_np(bits[0]).astype(np.float64), self.want)


class MergeLayerCase(StreamCase):
    name, covers = "merge_layer_link_probabilities", ("MergeLayer",)
    returns_without_waiting = True

    def shape(self):
        from tests import merge_layer_cases as mc
        return min(mc.ONE_PER_PATH, key=lambda c: c[2])[:3]

    def inputs(self):
        from tests import merge_layer_cases as mc
        a, b = mc.forward_inputs(*self.shape())
        return dict(a=np.array(a), b=np.array(b))

    def setup(self):
        from dyglib_amd import MergeLayer
        from tests import merge_layer_cases as mc
        dim, hidden, _ = self.shape()
        self.model = _load(MergeLayer(dim, dim, hidden, 1), {k: np.array(v) for k, v in mc.params(dim, hidden).items()}).to(DEV).eval()

    def call(self, t, hold=None):
        return [self.model.link_probabilities(t["a"], t["b"])], {}

    def check(self, bits, extra, tag):
        from tests import merge_layer_cases as mc
        from tests.parity import close
        close(_np(bits[0]), mc.forward_reference(*self.shape())[1], f"{self.name} {tag}", label="streams: merge head probabilities vs float64 reference")


class MetricsCase(StreamCase):
    name = "link_prediction_metrics_device"
    covers = ("link_prediction_metrics_device", "get_link_prediction_metrics", "get_node_classification_metrics")
    returns_without_waiting = True
    case = "odd37"

    def inputs(self):
        p, y = gc.build_metric_case(self.case)
        return dict(p=p, y=y)

    def setup(self):
        pass

    def call(self, t, hold=None):
        from dyglib_amd import link_prediction_metrics_device
        return list(link_prediction_metrics_device(t["p"], t["y"])), {}

    def check(self, bits, extra, tag):
        g = gc.load_golden("metrics")
        ap, auc, loss, status = (_np(x) for x in bits)
        ref = float(g[f"{self.case}|bce_loss"])
        assert int(status[0]) == 0
        assert abs(float(ap[0]) - float(g[f"{self.case}|average_precision"])) <= 1e-12 and abs(float(auc[0]) - float(g[f"{self.case}|roc_auc"])) <= 1e-12
        assert abs(float(loss[0]) - ref) <= 1e-6 * max(1.0, ref)


class _SamplerCase(StreamCase):
    graph = "gen_p1_l32"
    covers = ("NeighborSampler", "get_neighbor_sampler")

    def inputs(self):
        c = gc.build_case(self.graph)
        return dict(nodes=np.concatenate([c["src"], c["dst"]]).astype(np.int64), times=np.concatenate([c["times"], c["times"]]).astype(np.float64))

    def setup(self):
        from dyglib_amd import get_neighbor_sampler
        self.sampler = get_neighbor_sampler(gc.build_case(self.graph)["data"], "recent", seed=1, device=DEV)


class SamplerRecent(_SamplerCase):
    name = "sampler_get_historical_neighbors"
    returns_without_waiting = True
    k = gc.SAMPLER_KS[1]

    def call(self, t, hold=None):
        return list(self.sampler.get_historical_neighbors_device(t["nodes"], t["times"], self.k)), {}

    def check(self, bits, extra, tag):
        g = gc.load_golden(self.graph)
        for got, key in zip(bits, ("nbr", "eid", "ts")):
            np.testing.assert_array_equal(_np(got), g[f"recent{self.k}_{key}"])


class SamplerWindows(_SamplerCase):
    """padded_windows reads the largest window length back to size its outputs: the launch behind that read-back runs after the hold"""
    name = "sampler_padded_windows"

    def inputs(self):
        c = gc.build_case(self.graph)
        return dict(nodes=c["src"].astype(np.int64), times=c["times"].astype(np.float64))

    def call(self, t, hold=None):
        cfg = gc.build_case(self.graph)["cfg"]
        return list(self.sampler.padded_windows_device(t["nodes"], t["times"], cfg["patch_size"], cfg["max_input_sequence_length"])), {}

    def check(self, bits, extra, tag):
        g = gc.load_golden(self.graph)
        for got, key in zip(bits, ("src_pad_ids", "src_pad_eids", "src_pad_times")):
            np.testing.assert_array_equal(_np(got), g[key])


class CooccurrenceCase(StreamCase):
    name, covers = "count_nodes_appearances", ("count_nodes_appearances",)
    returns_without_waiting = True
    graph = "gen_p1_l32"

    def inputs(self):
        g = gc.load_golden(self.graph)
        return dict(src_ids=g["src_pad_ids"].astype(np.int64), dst_ids=g["dst_pad_ids"].astype(np.int64))

    def setup(self):
        pass

    def call(self, t, hold=None):
        from dyglib_amd import count_nodes_appearances
        return list(count_nodes_appearances(t["src_ids"], t["dst_ids"], device=DEV)), {}

    def check(self, bits, extra, tag):
        g = gc.load_golden(self.graph)
        np.testing.assert_array_equal(_np(bits[0]), g["src_counts"])
        np.testing.assert_array_equal(_np(bits[1]), g["dst_counts"])


# ---- one training step ---------------------------------------------------------------------------------------------------------------------------
P_DROP = 0.1


def _grads(model):
    return {n: (None if p.grad is None else _np(p.grad)) for n, p in model.named_parameters()}


class _TrainStep(_PairCase):
    """One training step, forward and backward, with `_fixed_dropout_seed` pinned and dropout P_DROP.  bits: the forward rows (the existing
    suite holds them to bit equality per seed).  extra: the parameter gradients -- atomic sums, so they are held, on either stream, to the
    oracle's autograd with the training path's own dropout masks at the scaled gradient bar; never to another run.  `hold`, when given, places
    a second blocker between the forward and the backward, so the backward's launches too are issued behind one."""
    seed = 0x1234568

    def loss(self, s, d):
        import torch
        G1, G2 = gc.grad_loss_weights(s.shape[0])
        return (s * torch.from_numpy(G1).to(s.device)).sum() + (d * torch.from_numpy(G2).to(d.device)).sum()

    def reset(self):
        self.model.zero_grad(set_to_none=True)

    def forward(self, t):
        raise NotImplementedError

    def call(self, t, hold=None):
        s, d = self.forward(t)
        w = self.weights(s)
        if hold is not None:
            hold()
        ((s * w[0]).sum() + (d * w[1]).sum()).backward()
        return [s.detach(), d.detach()], _grads(self.model)

    def weights(self, s):
        if not hasattr(self, "_w"):
            self._w = [_dev(g) for g in gc.grad_loss_weights(s.shape[0])]
            import torch
            torch.cuda.synchronize()
        return self._w

    def oracle(self):
        """(src_emb, dst_emb, {name: gradient or None}) of the oracle with this step's masks, computed once"""
        raise NotImplementedError

    def check(self, bits, extra, tag):
        from tests.parity import close, close_scaled
        if not hasattr(self, "_ref"):
            self._ref = self.oracle()
        ws, wd, ref = self._ref
        close(_np(bits[0]), ws, f"{self.name} {tag} src", label=f"streams: {self.name} forward with dropout vs oracle")
        close(_np(bits[1]), wd, f"{self.name} {tag} dst", label=f"streams: {self.name} forward with dropout vs oracle")
        for n, r in ref.items():
            if r is None:
                assert extra[n] is None, n
            else:
                close_scaled(extra[n], r, f"{self.name} {tag} grad {n}", label=f"streams: {self.name} gradients with dropout vs oracle autograd (scaled bar)")


class TgatTrain(_TrainStep):
    """a two-layer config of tests/test_tgat_configs_gpu.py with small feature widths, and its oracle with the training path's masks"""
    name, covers, label = "tgat_train_step", ("TGAT",), "dq32"

    @functools.cached_property
    def c(self):
        from tests.test_tgat_configs_gpu import _case
        c = _case(self.label)
        return dict(src=c["src"], dst=c["dst"], times=c["t"])

    def setup(self):
        from tests import test_tgat_configs_gpu as tg
        self.model = tg._model(self.label, train=True, p=P_DROP)
        self.k = tg.CONFIGS[self.label][4]

    def weights(self, s):
        from tests import test_tgat_configs_gpu as tg
        if not hasattr(self, "_w"):
            import torch
            self._w = [g.to(DEV) for g in tg._loss_weights(s.shape[0], s.shape[1])]
            torch.cuda.synchronize()
        return self._w

    def forward(self, t):
        return self.model.compute_src_dst_node_temporal_embeddings(t["src"], t["dst"], t["times"], num_neighbors=self.k)

    def oracle(self):
        from tests import test_tgat_configs_gpu as tg
        return tg._oracle(self.label, P_DROP)


class TclTrain(_TrainStep):
    name, covers = "tcl_train_step", ("TCL",)

    @functools.cached_property
    def c(self):
        from tests import tcl_cases as tc
        return tc.build_tcl_case("gen_k5_l1_h2")

    def setup(self):
        from tests.test_tcl_train_gpu import _train_case
        _, self.cfg, self.model = _train_case("gen_k5_l1_h2", P_DROP, self.seed)

    def forward(self, t):
        return self.model.compute_src_dst_node_temporal_embeddings(t["src"], t["dst"], t["times"], num_neighbors=self.cfg["K"])

    def oracle(self):
        from tests.test_tcl_grads_cpu import oracle_grads
        from tests.test_tcl_oracle_golden import OracleSampler
        c, cfg = self.c, self.cfg
        ws, wd, _, ref = oracle_grads(c, OracleSampler(c["data"], cfg["strategy"], cfg["sampler_seed"]), P_DROP, self.seed)
        return ws, wd, ref


class CawnTrain(_TrainStep):
    name, covers = "cawn_train_step", ("CAWN",)

    @functools.cached_property
    def c(self):
        from tests import cawn_cases as cc
        return cc.build_cawn_case("gen_w1_k5")

    def setup(self):
        from tests.test_cawn_train_gpu import _train_case
        _, self.cfg, self.model = _train_case("gen_w1_k5", P_DROP, self.seed)

    def forward(self, t):
        return self.model.compute_src_dst_node_temporal_embeddings(t["src"], t["dst"], t["times"], num_neighbors=self.cfg["k"])

    def oracle(self):
        from tests import cawn_oracle as cwo
        from tests.test_cawn_grads_cpu import oracle_grads
        c, cfg = self.c, self.cfg
        ws, wd, _, ref = oracle_grads(c, cwo.OracleSampler(c["data"], cfg["strategy"], cfg["sampler_seed"], cfg["scale"]), P_DROP, self.seed)
        return ws, wd, ref


class GraphMixerTrain(_TrainStep):
    name, covers = "graphmixer_train_step", ("GraphMixer",)

    @functools.cached_property
    def c(self):
        from tests import graphmixer_cases as gmc
        return gmc.build_graphmixer_case("gen_k10_g7")

    def setup(self):
        from tests.test_graphmixer_train_gpu import _train_case
        _, self.cfg, self.model = _train_case("gen_k10_g7", P_DROP, self.seed)

    def forward(self, t):
        return self.model.compute_src_dst_node_temporal_embeddings(t["src"], t["dst"], t["times"], num_neighbors=self.cfg["K"], time_gap=self.cfg["G"])

    def oracle(self):
        from tests.test_graphmixer_grads_cpu import case, oracle_grads
        ws, wd, _, ref = oracle_grads(case("gen_k10_g7"), P_DROP, self.seed)
        return ws, wd, ref


class _TwoPassTrainStep(_TrainStep):
    """DyGFormer and TGN have no oracle with dropout masks.  Their step runs twice in one call: with dropout P_DROP and the seed pinned --
    forward rows into `bits`, the backward run and its gradients required finite -- and with dropout 0, whose rows and gradients are held
    to the reference's own autograd fixtures (the same kernels, the mask a multiplication by one)."""

    def check_p0(self, bits, extra, tag):
        raise NotImplementedError

    def check(self, bits, extra, tag):
        for n, g in extra["dropout"].items():
            assert g is None or np.isfinite(g).all(), (self.name, tag, n)
        self.check_p0(bits, extra, tag)


class DygformerTrain(_TwoPassTrainStep):
    name, covers, graph = "dygformer_train_step", ("DyGFormer",), "hub_p4_l48"

    @functools.cached_property
    def c(self):
        return gc.build_case(self.graph)

    def setup(self):
        from tests.test_dygformer_gpu import build_model
        self.model, _ = build_model(self.c)
        self.model._fixed_dropout_seed = self.seed
        assert self.model.dropout == P_DROP

    def call(self, t, hold=None):
        m, w = self.model, None
        out = {}
        bits = []
        for p_tag in ("dropout", "p0"):
            m.train(p_tag == "dropout")          # eval mode with autograd recording: the training kernels at p = 0
            m.zero_grad(set_to_none=True)
            s, d = m.compute_src_dst_node_temporal_embeddings(t["src"], t["dst"], t["times"])
            w = self.weights(s)
            if hold is not None:
                hold()
            ((s * w[0]).sum() + (d * w[1]).sum()).backward()
            out[p_tag] = _grads(m)
            bits += [s.detach(), d.detach()]
        return bits, out

    def check_p0(self, bits, extra, tag):
        from tests.parity import close
        from tests.test_gradients_golden import _check
        g = gc.load_golden(self.graph)
        assert not any(bool((a == b).all()) for a, b in zip(bits[:2], bits[2:]))          # the dropout pass did drop
        close(_np(bits[2]), g["src_emb"], f"{self.name} {tag} p=0 src", label="streams: dygformer train forward vs reference")
        close(_np(bits[3]), g["dst_emb"], f"{self.name} {tag} p=0 dst", label="streams: dygformer train forward vs reference")
        _check(f"streams {self.name} {tag}", extra["p0"], gc.load_golden("grads_" + self.graph))


class TgnTrain(_TwoPassTrainStep):
    """the fixture protocol of tests/test_tgn_train_gpu.py: all batches but the last replayed without gradients, the last one as the negative call
    and the positive call with autograd, the bank restored from a backup before every pass"""
    name, covers, graph = "tgn_train_step", ("MemoryModel",), "tgn_gen_l2_k4"

    def inputs(self):
        b = gc.build_tgn_case(self.graph)["tgn_batches"][-1]
        return dict(src=b["src"].astype(np.int64), dst=b["dst"].astype(np.int64), neg=b["neg"].astype(np.int64), t=b["t"].astype(np.float64),
                    eid=b["eid"].astype(np.int64))

    def setup(self):
        import torch
        from tests.test_tgn_train_gpu import _model, _replay
        c = gc.build_tgn_case(self.graph)
        self.k = c["tgn_cfg"]["num_neighbors"]
        self.model = _model(c)
        self.model._fixed_dropout_seed = self.seed
        _replay(self.model, c, c["tgn_batches"][:-1])
        torch.cuda.synchronize()
        self.backup = self.model.memory_bank.backup_memory_bank()

    def reset(self):
        self.model.zero_grad(set_to_none=True)
        self.model.memory_bank.reload_memory_bank(self.backup)

    def call(self, t, hold=None):
        from tests import tgn_autograd as ta
        m = self.model
        out, bits = {}, []
        for p_tag in ("dropout", "p0"):
            self.reset()
            m.dropout = P_DROP if p_tag == "dropout" else 0.0
            embs = list(m.compute_src_dst_node_temporal_embeddings(t["src"], t["neg"], t["t"], edge_ids=None, edges_are_positive=False, num_neighbors=self.k))
            embs += list(m.compute_src_dst_node_temporal_embeddings(t["src"], t["dst"], t["t"], edge_ids=t["eid"], edges_are_positive=True, num_neighbors=self.k))
            if hold is not None:
                hold()
            ta.step_loss(*embs).backward()
            out[p_tag] = {n: g for n, g in _grads(m).items() if g is not None}
            bits += [e.detach() for e in embs]
        mb = m.memory_bank
        bits += [mb.node_memories.data.clone(), mb.node_last_updated_times.data.clone()]
        return bits, out

    def check_p0(self, bits, extra, tag):
        from tests.parity import close
        from tests.test_gradients_golden import _check
        g = gc.load_golden("grads_" + self.graph)
        assert sorted(extra["p0"]) == g["params_with_grad"].tolist()
        _check(f"streams {self.name} {tag}", extra["p0"], g)
        assert not any(bool((a == b).all()) for a, b in zip(bits[:4], bits[4:8]))          # the dropout pass did drop
        for got, key in zip(bits[4:8], ("neg_src_emb", "neg_dst_emb", "pos_src_emb", "pos_dst_emb")):
            close(_np(got), g[key], f"{self.name} {tag} p=0 {key}", label="streams: tgn train forward vs reference")
        close(_np(bits[8]), g["final_memory"], f"{self.name} {tag} memory", label="streams: tgn train forward vs reference")
        close(_np(bits[9]), g["final_last_update"], f"{self.name} {tag} last update", label="streams: tgn train forward vs reference")


def all_cases():
    return [DygformerInference(0), DygformerInference(1), DygformerMany(), TgatInference(), TclInference(), CawnInference(), GraphMixerInference(),
            TgnStep(), JodieStep(), DyrepStep(), EdgeBankCase(), MergeLayerCase(), MetricsCase(), SamplerRecent(), SamplerWindows(),
            CooccurrenceCase(), DygformerTrain(), TgatTrain(), TgnTrain(), TclTrain(), CawnTrain(), GraphMixerTrain()]


CASES = all_cases()
CASE_NAMES = [c.name for c in CASES]
TRAIN_BACKBONES = {"DyGFormer": "dygformer_train_step", "TGAT": "tgat_train_step", "MemoryModel": "tgn_train_step", "TCL": "tcl_train_step",
                   "CAWN": "cawn_train_step", "GraphMixer": "graphmixer_train_step"}
