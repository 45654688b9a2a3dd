"""DyGFormer's caches (dyglib_amd/_dygformer_caches.py) without a GPU: the full truth table of `pack_action`, and which of the model's
methods drop what.  tests/test_dygformer_caches_gpu.py holds the library calls each situation leads to."""
import itertools

import pytest
import torch

from dyglib_amd import synthetic as syn
from dyglib_amd._dygformer_caches import PackedWeights, ProjectedTables, pack_action
from dyglib_amd.temporal_csr import TemporalCSR

# (buffer exists, same key, same addresses, complete, training) -> action.  Written out from the rules of the kernel-ready copy:
# without a buffer everything is a full pack; an unchanged key keeps the copy, except that an inference call completes one the training
# path left incomplete; a changed key repacks in place when every address is where it was and packs otherwise.
F, T = False, True
TABLE = {
    (F, F, F, F, F): "pack", (F, F, F, F, T): "pack", (F, F, F, T, F): "pack", (F, F, F, T, T): "pack",
    (F, F, T, F, F): "pack", (F, F, T, F, T): "pack", (F, F, T, T, F): "pack", (F, F, T, T, T): "pack",
    (F, T, F, F, F): "pack", (F, T, F, F, T): "pack", (F, T, F, T, F): "pack", (F, T, F, T, T): "pack",
    (F, T, T, F, F): "pack", (F, T, T, F, T): "pack", (F, T, T, T, F): "pack", (F, T, T, T, T): "pack",
    (T, F, F, F, F): "pack", (T, F, F, F, T): "pack", (T, F, F, T, F): "pack", (T, F, F, T, T): "pack",
    (T, F, T, F, F): "repack", (T, F, T, F, T): "repack", (T, F, T, T, F): "repack", (T, F, T, T, T): "repack",
    (T, T, F, F, F): "complete", (T, T, F, F, T): "keep", (T, T, F, T, F): "keep", (T, T, F, T, T): "keep",
    (T, T, T, F, F): "complete", (T, T, T, F, T): "keep", (T, T, T, T, F): "keep", (T, T, T, T, T): "keep",
}


def test_pack_action_truth_table():
    combos = list(itertools.product((F, T), repeat=5))
    assert len(combos) == 32 and set(combos) == set(TABLE)
    for combo in combos:
        assert pack_action(*combo) == TABLE[combo], combo


@pytest.fixture()
def model():
    """the recipe of tests/test_dygformer_proj_tables_cpu.py: a small model constructed on the CPU"""
    from dyglib_amd import DyGFormer, NeighborSampler
    data, nf, ef = syn.make_bipartite_graph(5, 3, 20, seed=0)
    sampler = NeighborSampler(None, "recent", seed=0, csr=TemporalCSR.from_interactions(
        data.src_node_ids, data.dst_node_ids, data.edge_ids, data.node_interact_times), device="cpu")
    return DyGFormer(nf, ef, sampler, time_feat_dim=100, channel_embedding_dim=50, patch_size=2, num_layers=2, num_heads=2, dropout=0.1,
                     max_input_sequence_length=64, device="cpu")


def _filled(m):
    """put recognisable state into both caches, as a call on a GPU would have left it"""
    w, t = m._weights, m._tables
    assert isinstance(w, PackedWeights) and isinstance(t, ProjectedTables)
    w.buffer, w.key, w.addresses = torch.empty(4, dtype=torch.uint8), ("key",), (1, 2, 3)
    t.buffers = {"node": torch.empty(0), "edge": torch.empty(0)}
    return w, t, w.buffer


@pytest.mark.parametrize("what", ["train", "eval", "load_state_dict", "float", "invalidate_packed"])
def test_what_forgets_the_packed_key_keeps_buffer_and_addresses(model, what):
    w, t, buf = _filled(model)
    {"train": model.train, "eval": model.eval, "load_state_dict": lambda: model.load_state_dict(model.state_dict()),
     "float": model.float, "invalidate_packed": model.invalidate_packed}[what]()
    assert w.key is None and w.addresses == (1, 2, 3) and w.buffer is buf          # the next call repacks; it does not pack
    assert t.built == (set() if what == "invalidate_packed" else {"node", "edge"})


def test_a_table_assignment_drops_the_tables_and_nothing_else(model):
    w, t, buf = _filled(model)
    model.node_raw_features = model.node_raw_features
    assert t.built == set() and t.key is None
    assert w.key == ("key",) and w.addresses == (1, 2, 3) and w.buffer is buf
    assert model._weights is w and model._tables is t          # dropping empties the objects; it does not replace them
