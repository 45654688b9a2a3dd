"""Test support: ONE TGN call of the CPU oracle (oracle/tgn_oracle.py) under torch autograd.  The oracle's `tgn_forward` runs under no_grad;
its pieces (`_updated`, `_embed`) are plain differentiable torch, composed here the way the reference's graph is cut
(models/MemoryModel.py:87-168): the updated memories GRUCell(last message, stored memory) with grad-enabled parameter tensors (messages and
stored memories are constants), then the embedding module over updated memory + raw features.  The state commit of a positive call is the
oracle's own `tgn_forward` under no_grad.  Pinned to the reference's autograd by tests/test_tgn_grads_cpu.py (fixtures
tests/golden/grads_tgn_*.npz, tools/make_golden_tgn_grads.py); the GPU tests then use it off-fixture."""
import numpy as np
import torch

from oracle import dygformer_oracle as orc
from oracle import tgn_oracle as norc
from tests import golden_cases as gc

UNIFORM_CASE = "tgn_bip_l1_k10"


def grad_params(params: dict) -> dict:
    """every parameter but the memory bank as a grad-enabled tensor (the reference's memory bank is requires_grad=False)"""
    return {k: torch.from_numpy(np.array(v, copy=True)).requires_grad_("memory_bank" not in k) for k, v in params.items()}


def tgn_call(params, node_feat, edge_feat, adj, st, src, dst, times, edge_ids, positive, num_layers, num_neighbors, num_heads=2):
    """(src_emb, dst_emb) of one call with a graph back to `params`; a positive call then commits `st` as the oracle does."""
    nf = node_feat if isinstance(node_feat, torch.Tensor) else torch.from_numpy(node_feat)
    ef = edge_feat if isinstance(edge_feat, torch.Tensor) else torch.from_numpy(edge_feat)
    times = np.asarray(times, dtype=np.float64)
    node_ids = np.concatenate([src, dst])
    draws = _RecordedDraws() if positive else None
    if draws:
        draws.start()
    try:
        M_upd, _, _ = norc._updated(params, st, np.arange(st.M.shape[0]))                       # all nodes, MemoryModel.py:108-109
        emb = norc._embed(params, M_upd + nf, ef, adj, node_ids, np.concatenate([times, times]), num_layers, num_neighbors, num_heads)
    finally:
        if draws:
            draws.stop()
    if positive:
        # the commit alone matters here; the oracle recomputes the embeddings on the way: replay the neighbour draws it already made, so
        # that a random sampler's RandomState advances once per call, as in the reference
        draws.replay()
        try:
            norc.tgn_forward({k: v.detach() for k, v in params.items()}, nf, ef, adj, st, src, dst, times, edge_ids, True, num_layers, num_neighbors,
                             num_heads)
        finally:
            draws.stop()
    return emb[:len(src)], emb[len(src):]


class _RecordedDraws:
    """records what oracle.tgn_oracle.get_historical_neighbors_recent (possibly a test's random-strategy stand-in) returns, then plays it back"""

    def start(self):
        self.fn, self.log = norc.get_historical_neighbors_recent, []

        def rec(*a):
            out = self.fn(*a)
            self.log.append(out)
            return out
        norc.get_historical_neighbors_recent = rec

    def replay(self):
        it = iter(self.log)
        norc.get_historical_neighbors_recent = lambda *a: next(it)

    def stop(self):
        norc.get_historical_neighbors_recent = self.fn


def adjacency(data):
    return orc.OracleAdjacency(data.src_node_ids, data.dst_node_ids, data.edge_ids, data.node_interact_times)


def replay_prefix(params, c, adj, st, n_batches):
    """the first n_batches batches of a gc.TGN_CASES run under no_grad: negative call, then positive call"""
    cfg = c["tgn_cfg"]
    for b in c["tgn_batches"][:n_batches]:
        for dst, eid, pos in ((b["neg"], None, False), (b["dst"], b["eid"], True)):
            norc.tgn_forward(params, c["node_feat"], c["edge_feat"], adj, st, b["src"], dst, b["t"], eid, pos, cfg["num_layers"], cfg["num_neighbors"],
                             cfg["num_heads"])


def step_loss(ns, nd, ps, pd):
    """the fixtures' scalar: sum(neg_src G1) + sum(neg_dst G2) + sum(pos_src G2) + sum(pos_dst G1), G1, G2 = gc.grad_loss_weights(B)"""
    G1, G2 = (torch.from_numpy(g).to(ns.device) for g in gc.grad_loss_weights(ns.shape[0]))
    return (ns * G1).sum() + (nd * G2).sum() + (ps * G2).sum() + (pd * G1).sum()


def last_batch_grads(c, adj=None):
    """The fixture protocol on the oracle: all batches but the last under no_grad, the last with autograd.  Returns
    (params, loss, (neg_src, neg_dst, pos_src, pos_dst), state)."""
    cfg = c["tgn_cfg"]
    adj = adj if adj is not None else adjacency(c["data"])
    params = grad_params(c["tgn_params"])
    st = norc.TgnState(c["node_feat"].shape[0], c["node_feat"].shape[1])
    plain = {k: v.detach() for k, v in params.items()}
    replay_prefix(plain, c, adj, st, len(c["tgn_batches"]) - 1)
    b = c["tgn_batches"][-1]
    args = (cfg["num_layers"], cfg["num_neighbors"], cfg["num_heads"])
    ns, nd = tgn_call(params, c["node_feat"], c["edge_feat"], adj, st, b["src"], b["neg"], b["t"], None, False, *args)
    ps, pd = tgn_call(params, c["node_feat"], c["edge_feat"], adj, st, b["src"], b["dst"], b["t"], b["eid"], True, *args)
    loss = step_loss(ns, nd, ps, pd)
    loss.backward()
    return params, loss, (ns, nd, ps, pd), st


def uniform_draw(sampler, adj):
    """A stand-in for oracle.tgn_oracle.get_historical_neighbors_recent that samples `uniform` (utils/utils.py:149-199): history lengths
    from the oracle, positions from the host sampler's RandomState replay."""
    def draw(_, ids, t, k):
        ids = np.asarray(ids, dtype=np.int64)
        hist = np.array([len(orc.find_neighbors_before(adj, v, tt)[0]) for v, tt in zip(ids, t)], dtype=np.int32)
        sel = sampler._draw_host(ids, hist, k)
        out_n, out_e, out_t = np.zeros((len(ids), k), np.int64), np.zeros((len(ids), k), np.int64), np.zeros((len(ids), k), np.float32)
        for r in np.nonzero(hist > 0)[0]:
            nb, eb, tb = adj.row(int(ids[r]))
            out_n[r], out_e[r], out_t[r] = nb[sel[r]], eb[sel[r]], tb[sel[r]]
        return out_n, out_e, out_t
    return draw
