"""What DyGFormer's caches make the library do, and the padded lengths of a training call.

a. A call trace.  `model._lib` is replaced by a proxy that records every dygnn_dygformer_pack, dygnn_dygformer_repack (with its
   fused_only argument) and dygnn_dygformer_project_table (with its channel) and forwards everything.  A sequence of situations -- first
   call, unchanged weights, in-place update, training forward, train() / eval(), load_state_dict, invalidate_packed(), a parameter at a new
   address -- must lead to exactly the calls written out here (dyglib_amd/_dygformer_caches.py: pack_action), and every inference result is
   held to the oracle at the project's bar: a full pack after every optimizer step (it synchronises its stream), or a completing repack
   that is skipped, changes no result that any other test would see.
b. `_seq_lens_groups`, the one routine that computes a call's padded lengths on the side stream, for one call ([1, B] views) and a set of
   two, from host and from device inputs, against the lengths of the oracle's windows.  The slices are chosen (and asserted, from the oracle
   alone, in a test that needs no GPU) so that the two sides pad differently, `longest window + 1` is no multiple of the patch size, and
   the two calls of a set pad differently."""
import numpy as np
import pytest
import torch

from oracle import dygformer_oracle as orc
from tests import golden_cases as gc

PACK, REPACK, REPACK_FUSED_ONLY = "pack", "repack", "repack fused_only"
TABLES = ["project node", "project edge"]


class _Recorder:
    """stands where the ctypes library stands; `calls` is emptied by whoever reads it"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        tag = {"dygnn_dygformer_pack": lambda a: PACK, "dygnn_dygformer_repack": lambda a: REPACK_FUSED_ONLY if a[4] else REPACK,
               "dygnn_dygformer_project_table": lambda a: "project " + ("node", "edge")[a[2]]}.get(name)
        if tag is None:
            return fn

        def recorded(*args):
            self.calls.append(tag(args))
            return fn(*args)
        return recorded

    def take(self):
        calls, self.calls = self.calls, []
        return calls


@pytest.mark.gpu
def test_library_calls_of_every_cache_situation(monkeypatch):
    from tests.test_streams_gpu import _Fresh
    monkeypatch.setenv("DYGNN_PROJ_TABLES", "1")
    monkeypatch.delenv("DYGNN_POOLED_TAIL", raising=False)
    f = _Fresh(9300)
    m = f.model
    rec = m._lib = _Recorder(m._lib)

    def infer(i, step, want):
        out = f.infer(i)
        got = rec.take()
        print(f"cache trace, step {step}: {got}")
        assert got == want, f"step {step}"
        torch.cuda.synchronize()
        f.check(out, i, f"cache trace, step {step}")

    infer(0, "1 first call", [PACK] + TABLES)
    infer(0, "2 the same call again", [])
    f.update(1)
    infer(1, "3 in-place update", [REPACK] + TABLES)
    f.update(2)
    with pytest.warns(RuntimeWarning, match="autograd recording"):
        f.train_forward(0)                           # eval mode with autograd recording: the training path, no train() / eval() switch
    assert rec.take() == [REPACK_FUSED_ONLY], "step 4, the training forward"
    infer(0, "4 after a training forward", [REPACK] + TABLES)          # the completing repack; the tables follow the generation of the first
    infer(1, "4b again", [])
    m.train()
    m.eval()
    infer(1, "5 train(); eval()", [REPACK] + TABLES)
    m.load_state_dict(m.state_dict())
    infer(0, "6 load_state_dict", [REPACK] + TABLES)
    m.invalidate_packed()
    assert m._lib is rec and rec.take() == []
    infer(1, "7 invalidate_packed()", [REPACK] + TABLES)
    p = m.output_layer.bias
    p.data = p.data.clone()                          # the same values at another address: the descriptors in the buffer are stale
    infer(0, "8 a parameter's storage replaced", [PACK] + TABLES)
    infer(1, "8b again", [])
    assert f.params_match_the_model()


# ---- b. padded lengths ------------------------------------------------------------------------------------------------------------------
LENGTH_CASES = [("hub_p4_l48", slice(0, 12)), ("hub_p4_l48", slice(0, 24)), ("bip_p2_l64", slice(0, 5)), ("bip_p2_l64", slice(0, 40))]


def _oracle_lengths(name, sl):
    """-> (case, [N = 2, B] host inputs: the fixture's positive and negative call, per call (S_src, S_dst), per call and side longest window)"""
    c = gc.build_case(name)
    d, P, L = c["data"], c["cfg"]["patch_size"], c["cfg"]["max_input_sequence_length"]
    adj = orc.OracleAdjacency(d.src_node_ids, d.dst_node_ids, d.edge_ids, d.node_interact_times)
    src, dst, neg, t = c["src"][sl], c["dst"][sl], c["neg_dst"][sl], c["times"][sl]
    assert 0 < len(src) <= 40
    padded, longest = [], []
    for ids in ((src, dst), (src, neg)):
        padded.append(tuple(orc.first_hop_windows(adj, x, t, P, L)[0].shape[1] for x in ids))
        longest.append(tuple(max(min(len(w), L - 1) for w in orc.get_all_first_hop_neighbors(adj, x, t)[0]) for x in ids))
    return c, [np.stack([src, src]), np.stack([dst, neg]), np.stack([t, t])], padded, longest


def test_the_length_cases_cover_what_they_are_meant_to():
    seen = set()
    for name, sl in LENGTH_CASES:
        c, _, padded, longest = _oracle_lengths(name, sl)
        P = c["cfg"]["patch_size"]
        seen |= {"sides differ"} if any(a != b for a, b in padded) else set()
        seen |= {"not a multiple of P"} if any((w + 1) % P for row in longest for w in row) else set()
        seen |= {"calls differ"} if padded[0] != padded[1] else set()
    assert seen == {"sides differ", "not a multiple of P", "calls differ"}


@pytest.mark.gpu
@pytest.mark.parametrize("name,sl", LENGTH_CASES, ids=[f"{n}-{s.stop}" for n, s in LENGTH_CASES])
def test_padded_lengths_equal_the_oracles(name, sl):
    from tests.test_dygformer_gpu import build_model
    c, host, padded, _ = _oracle_lengths(name, sl)
    model, _ = build_model(c)
    dev = torch.device("cuda:0")
    devt = [torch.from_numpy(x).to(dev) for x in host]
    assert model._seq_lens_groups(*host, *devt, dev) == padded                   # the set of two, host inputs
    assert model._seq_lens_groups(*devt, *devt, dev) == padded                   # ... device inputs
    for i in (0, 1):                                                             # each call alone, as [1, B]
        one_host, one_dev = [x[i:i + 1] for x in host], [x[i:i + 1] for x in devt]
        assert model._seq_lens_groups(*one_host, *one_dev, dev) == [padded[i]]
        assert model._seq_lens_groups(*one_dev, *one_dev, dev) == [padded[i]]
