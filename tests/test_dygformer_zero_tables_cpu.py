"""The "all zero" bits of DyGFormer's feature tables (table_flags of dygnn_dygformer_forward_tables): established by the class from the
arrays it is given, per table, and again when a table is assigned.  No kernel is launched here; that the header, _capi and the library
agree on the new entry point is tests/test_capi_cpu.py::test_header_symbols_are_exported_and_bound."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from dyglib_amd import _build, _capi, synthetic as syn
from dyglib_amd.temporal_csr import TemporalCSR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE, EDGE = _capi.TABLE_NODE_ZERO, _capi.TABLE_EDGE_ZERO


@pytest.fixture(scope="module")
def graph():
    _build.build(verbose=False)
    from dyglib_amd import NeighborSampler
    data, nf, ef = syn.make_bipartite_graph(5, 3, 20, seed=0)
    sampler = NeighborSampler(None, "recent", seed=0, csr=TemporalCSR.from_interactions(
        data.src_node_ids, data.dst_node_ids, data.edge_ids, data.node_interact_times), device="cpu")
    return nf, ef, sampler


def _model(nf, ef, sampler):
    from dyglib_amd import DyGFormer
    return DyGFormer(nf, ef, sampler, time_feat_dim=100, channel_embedding_dim=50, patch_size=2, num_layers=2, num_heads=2,
                     dropout=0.1, max_input_sequence_length=64, device="cpu")


def _last_element_set(table):
    t = np.zeros_like(table)
    t[-1, -1] = 1e-30
    return t


def test_bits_follow_the_tables_given_to_the_constructor(graph):
    nf, ef, sampler = graph
    assert not nf.any() and ef.any()                                   # the generator's tables: zero node features, random edge features
    assert _model(nf, ef, sampler).table_flags == NODE
    assert _model(nf, np.zeros_like(ef), sampler).table_flags == NODE | EDGE
    assert _model(_last_element_set(nf), ef, sampler).table_flags == 0                     # one non-zero element, the last of the last row
    assert _model(nf, _last_element_set(ef), sampler).table_flags == NODE
    assert _model(_last_element_set(nf), np.zeros_like(ef), sampler).table_flags == EDGE
    neg0 = np.full_like(nf, -0.0)                                      # -0.0 is zero: w * -0.0 adds nothing to a bias either
    assert _model(neg0, ef, sampler).table_flags == NODE


def test_assigning_a_table_establishes_its_bit_again(graph):
    nf, ef, sampler = graph
    m = _model(nf, ef, sampler)
    assert m.table_flags == NODE
    m.node_raw_features = torch.from_numpy(_last_element_set(nf))
    assert m.table_flags == 0 and m.node_raw_features[-1, -1] != 0
    m.edge_raw_features = torch.zeros_like(m.edge_raw_features)
    assert m.table_flags == EDGE
    m.node_raw_features = torch.zeros_like(m.node_raw_features)
    assert m.table_flags == NODE | EDGE
    # the tables stay plain attributes: not parameters, not buffers, not in the state_dict (models/DyGFormer.py:32-33)
    assert not any("raw_features" in k for k in m.state_dict()) and not any("raw_features" in k for k, _ in m.named_buffers())


def test_entry_point_is_bound_with_a_trailing_flags_word_and_the_abi_moved(graph):
    lib = _capi.load()
    restype, argtypes = _capi.SIGNATURES["dygnn_dygformer_forward_tables"]
    assert restype is C.c_int and argtypes[:-1] == _capi.SIGNATURES["dygnn_dygformer_forward"][1] and argtypes[-1] is C.c_uint32
    header = open(os.path.join(ROOT, "include", "dygnn.h")).read()
    assert int(re.search(r"#define DYGNN_TABLE_NODE_ZERO (\d+)u", header).group(1)) == NODE
    assert int(re.search(r"#define DYGNN_TABLE_EDGE_ZERO (\d+)u", header).group(1)) == EDGE
    assert lib.dygnn_abi_version() == _capi.ABI_VERSION >= 18
    # an unknown bit is rejected before anything is launched (no GPU here: the call must not get further than its argument checks)
    cfg = _capi.DygformerConfig(172, 172, 100, 50, 2, 2, 2, 64)
    rc = lib.dygnn_dygformer_forward_tables(C.byref(cfg), None, None, None, None, None, None, None, None, 0, 0, 0, None, None, None, 0, None, 0, None, 4)
    assert rc == -1 and b"table_flags" in lib.dygnn_last_error()
