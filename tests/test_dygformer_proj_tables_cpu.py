"""Projected feature tables of the DyGFormer inference path without a GPU: the size function against its formula, the class's choice of
which channel gets a table (all-zero bit, size cap, impl, DYGNN_PROJ_TABLES) with the flag bits it passes, and the agreement of header,
bindings and exports for the new entry points.  No kernel is launched: every library call here fails validation first."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from dyglib_amd import _capi, synthetic as syn
from dyglib_amd.temporal_csr import TemporalCSR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dygnn_dygformer_projected_bytes", "dygnn_dygformer_project_table", "dygnn_dygformer_forward_projected")


@pytest.mark.parametrize("P,L", [(1, 32), (2, 64), (8, 512)])
def test_projected_bytes_is_rows_times_slots_times_a_64_float_segment(P, L):
    lib = _capi.load()
    cfg = _capi.DygformerConfig(172, 172, 100, 50, P, 2, 2, L)
    for rows in (1, 7, 157475):
        assert lib.dygnn_dygformer_projected_bytes(C.byref(cfg), rows) == rows * P * _capi.PROJ_ROW_FLOATS * 4
    assert lib.dygnn_dygformer_projected_bytes(C.byref(cfg), 0) == 0 and lib.dygnn_dygformer_projected_bytes(C.byref(cfg), -3) == 0
    assert lib.dygnn_dygformer_projected_bytes(None, 5) == 0
    bad = _capi.DygformerConfig(172, 172, 100, 50, P, 2, 3, L)          # 200 % 3 != 0
    assert lib.dygnn_dygformer_projected_bytes(C.byref(bad), 5) == 0
    other = _capi.DygformerConfig(172, 172, 100, 48, P, 2, 2, L)        # a channel width the fused kernel does not run: nothing to project for
    assert lib.dygnn_dygformer_projected_bytes(C.byref(other), 5) == 0


def test_header_bindings_and_exports_agree():
    lib = _capi.load()
    header = open(os.path.join(ROOT, "include", "dygnn.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _capi.SIGNATURES and f" {name}(" in header
    assert int(re.search(r"#define DYGNN_TABLE_NODE_PROJ (\d+)u", header).group(1)) == _capi.TABLE_NODE_PROJ == 4
    assert int(re.search(r"#define DYGNN_TABLE_EDGE_PROJ (\d+)u", header).group(1)) == _capi.TABLE_EDGE_PROJ == 8
    restype, argtypes = _capi.SIGNATURES["dygnn_dygformer_forward_projected"]
    assert restype is C.c_int and argtypes[:-2] == _capi.SIGNATURES["dygnn_dygformer_forward_tables"][1] and argtypes[-2:] == [C.c_void_p, C.c_void_p]


def test_argument_checks_come_before_any_launch():
    lib = _capi.load()
    cfg = _capi.DygformerConfig(172, 172, 100, 50, 2, 2, 2, 64)
    fwd = lambda flags, pn, pe: lib.dygnn_dygformer_forward_projected(C.byref(cfg), None, None, None, None, None, None, None, None, 0, 0, 0, None, None,
                                                                     None, 0, None, 0, None, flags, pn, pe)
    assert fwd(16, None, None) == -1 and b"table_flags" in lib.dygnn_last_error()
    assert fwd(_capi.TABLE_EDGE_PROJ, None, None) == -1 and b"edge_proj is NULL" in lib.dygnn_last_error()
    assert fwd(_capi.TABLE_NODE_PROJ, None, 1 << 20) == -1 and b"node_proj is NULL" in lib.dygnn_last_error()
    assert fwd(_capi.TABLE_EDGE_PROJ, None, (1 << 20) + 4) == -1 and b"16-byte aligned" in lib.dygnn_last_error()
    # the older entry point still refuses the new bits: it has no pointer to go with them
    rc = lib.dygnn_dygformer_forward_tables(C.byref(cfg), None, None, None, None, None, None, None, None, 0, 0, 0, None, None, None, 0, None, 0, None, 8)
    assert rc == -1 and b"table_flags" in lib.dygnn_last_error()
    w = _capi.DygformerWeights()
    assert lib.dygnn_dygformer_project_table(C.byref(cfg), C.byref(w), 2, None, 5, None, 0, None) == -1 and b"channel" in lib.dygnn_last_error()
    assert lib.dygnn_dygformer_project_table(C.byref(cfg), C.byref(w), 1, None, 5, None, 0, None) == -1 and b"null projection weights" in lib.dygnn_last_error()
    w.proj_node_w = w.proj_edge_w = 1 << 20
    assert lib.dygnn_dygformer_project_table(C.byref(cfg), C.byref(w), 1, None, 5, None, 0, None) == -1 and b"null table" in lib.dygnn_last_error()
    need = 5 * 2 * 64 * 4
    assert lib.dygnn_dygformer_project_table(C.byref(cfg), C.byref(w), 1, 1 << 20, 5, 1 << 21, need - 1, None) == -4 and b"too small" in lib.dygnn_last_error()


@pytest.fixture()
def model():
    from dyglib_amd import DyGFormer, NeighborSampler
    data, nf, ef = syn.make_bipartite_graph(5, 3, 20, seed=0)
    sampler = NeighborSampler(None, "recent", seed=0, csr=TemporalCSR.from_interactions(
        data.src_node_ids, data.dst_node_ids, data.edge_ids, data.node_interact_times), device="cpu")
    return DyGFormer(nf, ef, sampler, time_feat_dim=100, channel_embedding_dim=50, patch_size=2, num_layers=2, num_heads=2, dropout=0.1,
                     max_input_sequence_length=64, device="cpu")


def test_which_channel_gets_a_table_and_the_bits_that_say_so(model, monkeypatch):
    monkeypatch.delenv("DYGNN_PROJ_TABLES", raising=False)
    NODE, EDGE = _capi.TABLE_NODE_PROJ, _capi.TABLE_EDGE_PROJ
    rows_e, rows_n = model.edge_raw_features.shape[0], model.node_raw_features.shape[0]
    per_row = 2 * 64 * 4
    assert model.proj_table_max_bytes == 1 << 30
    # the bipartite graph's node table is all zero: it builds nothing; its edge table is not
    assert model.table_flags == _capi.TABLE_NODE_ZERO
    plan = model._proj_plan()
    assert plan == {"edge": rows_e * per_row} and model._proj_flags(plan) == EDGE
    model.node_raw_features = torch.ones_like(model.node_raw_features)
    plan = model._proj_plan()
    assert plan == {"node": rows_n * per_row, "edge": rows_e * per_row} and model._proj_flags(plan) == NODE | EDGE
    # the cap is per table: the larger table keeps the MFMA path, the other does not
    big, small = ("edge", "node") if rows_e > rows_n else ("node", "edge")
    model.proj_table_max_bytes = max(rows_e, rows_n) * per_row - 1
    assert set(model._proj_plan()) == {small}
    model.proj_table_max_bytes = 0
    assert model._proj_plan() == {}
    monkeypatch.setenv("DYGNN_PROJ_TABLES", "1")                   # forced: whatever the size
    assert set(model._proj_plan()) == {"node", "edge"}
    monkeypatch.setenv("DYGNN_PROJ_TABLES", "0")
    model.proj_table_max_bytes = 1 << 30
    assert model._proj_plan() == {} and model._proj_flags({}) == 0
    monkeypatch.delenv("DYGNN_PROJ_TABLES")
    for impl, want in ((1, set()), (3, set()), (0, {"node", "edge"})):          # a pinned implementation keeps its own projection
        model.impl = impl
        assert set(model._proj_plan()) == want
    model.edge_raw_features = torch.zeros_like(model.edge_raw_features)
    assert set(model._proj_plan()) == {"node"}
    assert model.table_flags == _capi.TABLE_EDGE_ZERO              # the zero bits are untouched by all of this


def test_assigning_a_table_or_invalidating_the_weights_drops_the_projected_tables(model):
    held = {"node": torch.empty(0), "edge": torch.empty(0)}
    model._tables.buffers = dict(held)
    assert model._tables.built == {"node", "edge"}
    model.edge_raw_features = model.edge_raw_features
    assert model._tables.built == set()
    model._tables.buffers = dict(held)
    model.invalidate_packed()
    assert model._tables.built == set()
