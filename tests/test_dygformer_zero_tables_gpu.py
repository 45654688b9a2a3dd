"""dygnn_dygformer_forward_tables: a feature table the caller declares all zero leaves the patch projection of the fused kernel.

For finite weights the flagged call on a zero table must return the BITS of the unflagged call (adding w * 0 to the projection bias
changes nothing; the weights of syn.make_dygformer_params have no -0.0 bias, the one documented exception), in every inference shape of
the kernel: the four-wave kernel of small calls, the eight-wave kernel with a half-full last workgroup, the 128-token kernel, the
positive / negative pairing inside a workgroup, several groups, and the tapped (PL = 2) form.  Chunk counts of the dropped channel cover
whole groups of four, remainders 2 and 3, and a channel that spans more than one LDS half.  The calls go through _capi so that the flags
are the test's, not the class's."""
import ctypes as C

import numpy as np
import pytest
import torch

from dyglib_amd import _capi
from dyglib_amd import synthetic as syn
from oracle import dygformer_oracle as orc
from tests.parity import close_scaled

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NODE, EDGE = _capi.TABLE_NODE_ZERO, _capi.TABLE_EDGE_ZERO


def _graph(edge_kind="normal", node_random=False):
    data, nf, ef = syn.make_bipartite_graph(60, 20, 3000, seed=31, edge_feat_kind=edge_kind)      # zero node table, as every reference dataset
    if node_random:
        nf[1:] = np.random.RandomState(3).standard_normal(nf[1:].shape).astype(np.float32) * 0.3
    return data, nf, ef


@pytest.fixture(scope="module")
def graphs():
    return {"node0": _graph(), "both0": _graph("zeros"), "edge0": _graph("zeros", node_random=True)}


_MODELS = {}


def _model(graphs, which, L, P):
    from dyglib_amd import DyGFormer, get_neighbor_sampler
    key = (which, L, P)
    if key not in _MODELS:
        data, nf, ef = graphs[which]
        params = syn.make_dygformer_params(11, patch_size=P)
        sampler = get_neighbor_sampler(data, "recent", seed=1, device=DEV)
        m = DyGFormer(nf, ef, sampler, 100, 50, patch_size=P, num_layers=2, num_heads=2, dropout=0.1, max_input_sequence_length=L, device=DEV)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        m = m.to(DEV).eval()
        m.impl = 3
        _MODELS[key] = (m, params)
    return _MODELS[key]


def _forward(model, src, dst, t, flags, group_size=0, pair_stride=0, taps=None):
    dev = model._device()
    s, d, tm = (model._to_dev(x, ty, dev) for x, ty in ((src, torch.int64), (dst, torch.int64), (t, torch.float64)))
    B = s.numel()
    weights, packed = model._packed_weights(dev)
    ws = model._workspace_for(B, dev)
    out_src = torch.empty((B, model.node_feat_dim), dtype=torch.float32, device=dev)
    out_dst = torch.empty_like(out_src)
    ts = model._make_taps(taps, B, dev) if taps is not None else None
    rc = model._lib.dygnn_dygformer_forward_tables(
        C.byref(model._cfg), C.byref(weights), packed.data_ptr(), model.neighbor_sampler.csr.on_device(dev),
        model.node_raw_features.data_ptr(), model.edge_raw_features.data_ptr(), s.data_ptr(), d.data_ptr(), tm.data_ptr(), B, group_size, pair_stride,
        out_src.data_ptr(), out_dst.data_ptr(), ws.data_ptr(), ws.numel(), C.byref(ts) if ts is not None else None, 3, _capi.current_stream_ptr(), flags)
    _capi.check(rc)
    torch.cuda.synchronize()
    return out_src, out_dst


def _last(data, B):
    idx = np.arange(data.num_interactions - B, data.num_interactions)
    return data.src_node_ids[idx], data.dst_node_ids[idx], data.node_interact_times[idx]


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("B", [5, 259])                             # four-wave kernel; eight-wave kernel, last workgroup half full
@pytest.mark.parametrize("L,P", [(64, 2), (32, 1), (48, 4)])        # node chunks 22 (remainder 2), 11 (remainder 3), 43 (more than one half)
def test_flagged_call_returns_the_bits_of_the_unflagged_call(graphs, L, P, B):
    model, _ = _model(graphs, "node0", L, P)
    assert model.table_flags == NODE
    src, dst, t = _last(graphs["node0"][0], B)
    plain = _forward(model, src, dst, t, 0)
    assert _same(_forward(model, src, dst, t, NODE), plain)
    assert float(plain[0].abs().max()) > 0 and torch.isfinite(plain[0]).all()
    # the class passes its own bits: the same result
    with torch.no_grad():
        assert _same(model.compute_src_dst_node_temporal_embeddings(src, dst, t), plain)


@pytest.mark.parametrize("group_size", [130, 65])           # one group per call; two groups per call
def test_positive_and_negative_calls_in_one_workgroup(graphs, group_size):
    model, _ = _model(graphs, "node0", 64, 2)
    data = graphs["node0"][0]
    src, dst, t = _last(data, 130)
    neg = syn.random_negative_dst(np.random.RandomState(4), np.unique(data.dst_node_ids), 130)
    src2, dst2, t2 = np.concatenate([src, src]), np.concatenate([dst, neg]), np.concatenate([t, t])
    plain = _forward(model, src2, dst2, t2, 0, group_size, 130)
    assert _same(_forward(model, src2, dst2, t2, NODE, group_size, 130), plain)
    assert _same(_forward(model, src2, dst2, t2, NODE, group_size, 0), plain)       # ... and of the unpaired flagged launch


def test_both_tables_zero_in_the_128_token_kernel(graphs):
    model, _ = _model(graphs, "both0", 512, 8)
    assert model.table_flags == NODE | EDGE
    src, dst, t = _last(graphs["both0"][0], 3)
    plain = _forward(model, src, dst, t, 0)
    for flags in (NODE | EDGE, NODE, EDGE):
        assert _same(_forward(model, src, dst, t, flags), plain), flags


@pytest.mark.parametrize("L,P,B", [(64, 2, 5), (64, 2, 259), (512, 8, 3)])
def test_zero_edge_table_alone(graphs, L, P, B):
    model, _ = _model(graphs, "edge0", L, P)
    assert model.table_flags == EDGE
    src, dst, t = _last(graphs["edge0"][0], B)
    assert _same(_forward(model, src, dst, t, EDGE), _forward(model, src, dst, t, 0))


def test_tapped_call(graphs):
    model, _ = _model(graphs, "node0", 64, 2)
    src, dst, t = _last(graphs["node0"][0], 7)
    tp, tf = {}, {}
    plain = _forward(model, src, dst, t, 0, taps=tp)
    assert _same(_forward(model, src, dst, t, NODE, taps=tf), plain)
    assert torch.equal(tf["encoder_input"], tp["encoder_input"]) and float(tp["encoder_input"].abs().max()) > 0
    assert torch.equal(tf["layer_outputs"][-1], tp["layer_outputs"][-1]) and float(tp["layer_outputs"][-1].abs().max()) > 0
    assert _same(plain, _forward(model, src, dst, t, NODE))                        # the tapped (full stream) and the pooled form agree


def test_flagged_call_against_the_oracle(graphs):
    model, params = _model(graphs, "node0", 64, 2)
    data, nf, ef = graphs["node0"]
    src, dst, t = _last(data, 24)
    adj = orc.OracleAdjacency(data.src_node_ids, data.dst_node_ids, data.edge_ids, data.node_interact_times)
    with torch.no_grad():
        os_, od = orc.dygformer_forward(params, nf, ef, adj, src, dst, t, 2, 64)
    gs, gd = _forward(model, src, dst, t, NODE)
    close_scaled(gs.cpu().numpy(), os_.numpy(), "zero node table, flagged: src emb")
    close_scaled(gd.cpu().numpy(), od.numpy(), "zero node table, flagged: dst emb")


def test_unknown_flag_bit_is_an_error(graphs):
    model, _ = _model(graphs, "node0", 64, 2)
    src, dst, t = _last(graphs["node0"][0], 5)
    with pytest.raises(Exception):
        _forward(model, src, dst, t, 4)
