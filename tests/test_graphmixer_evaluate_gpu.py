"""evaluate_model_link_prediction("GraphMixer", ...) on an MI355X against the reference's own run of its evaluation loop
(tests/golden/eval_graphmixer.npz, tools/make_golden_graphmixer.py): the negative draws bit-equal, the per-batch loss / AUC / AP within the bars
of tests/test_evaluate.py::test_evaluation_loop_matches_reference (1e-5 / 2e-3 / 1e-2), one step per call and 32 steps per call."""
import numpy as np
import pytest

from tests import golden_cases as gc
from tests import graphmixer_cases as gmc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def build():
    import torch
    from dyglib_amd import GraphMixer, MergeLayer, get_neighbor_sampler
    c = gmc.build_eval_case()
    cfg = c["gm_cfg"]
    sampler = get_neighbor_sampler(c["data"], "recent", seed=1, device=DEV)
    bb = GraphMixer(c["node_feat"], c["edge_feat"], sampler, cfg["time_feat_dim"], num_tokens=cfg["K"], num_layers=cfg["layers"], dropout=0.1, device=DEV)
    bb.load_state_dict({k: torch.from_numpy(v) for k, v in c["gm_params"].items()}, strict=True)
    merge = MergeLayer(172, 172, 172, 1)
    merge.load_state_dict({k: torch.from_numpy(v) for k, v in c["mparams"].items()}, strict=True)
    return c, cfg, sampler, torch.nn.Sequential(bb, merge).to(DEV)


@pytest.mark.parametrize("fuse", [1, 32])
def test_evaluation_loop_matches_reference(fuse):
    import torch
    from dyglib_amd import Data, NegativeEdgeSampler, evaluate_model_link_prediction, get_idx_data_loader
    c, cfg, sampler, model = build()
    g = gc.load_golden("eval_graphmixer")
    d = c["data"]
    first, last = gc.eval_indices(d.num_interactions)
    sl = slice(first, last)
    eval_data = Data(d.src_node_ids[sl], d.dst_node_ids[sl], d.node_interact_times[sl], d.edge_ids[sl], d.labels[sl])
    loader = get_idx_data_loader(list(range(last - first)), cfg["batch"], shuffle=False)
    neg = NegativeEdgeSampler(src_node_ids=d.src_node_ids, dst_node_ids=d.dst_node_ids, seed=gc.EVAL_NEG_SEED)
    draws = []
    sample = neg.sample
    neg.sample = lambda *a, **k: (lambda r: (draws.append(r[1]), r)[1])(sample(*a, **k))          # record what the loop draws
    losses, metrics = evaluate_model_link_prediction(model_name="GraphMixer", model=model, neighbor_sampler=sampler, evaluate_idx_data_loader=loader,
                                                     evaluate_neg_edge_sampler=neg, evaluate_data=eval_data, loss_func=torch.nn.BCELoss(),
                                                     num_neighbors=cfg["K"], time_gap=cfg["G"], fuse_batches=fuse)
    assert np.array_equal(np.concatenate(draws), g["neg_dst"])
    assert len(losses) == len(metrics) == len(g["losses"]) and all(isinstance(x, float) for x in losses)
    errs = (np.abs(np.array(losses) - g["losses"]).max(), np.abs(np.array([m["roc_auc"] for m in metrics]) - g["roc_auc"]).max(),
            np.abs(np.array([m["average_precision"] for m in metrics]) - g["average_precision"]).max())
    print(f"fuse_batches={fuse}: max |loss err| {errs[0]:.3e}, |auc err| {errs[1]:.3e}, |ap err| {errs[2]:.3e}")
    assert errs[0] <= 1e-5
    assert errs[1] <= 2e-3
    assert errs[2] <= 1e-2


def test_time_gap_reaches_the_model():
    """the loop passes time_gap through: a different window gives different losses"""
    import torch
    from dyglib_amd import Data, NegativeEdgeSampler, evaluate_model_link_prediction, get_idx_data_loader
    c, cfg, sampler, model = build()
    d = c["data"]
    first, last = gc.eval_indices(d.num_interactions)
    sl = slice(first, first + 80)
    eval_data = Data(d.src_node_ids[sl], d.dst_node_ids[sl], d.node_interact_times[sl], d.edge_ids[sl], d.labels[sl])
    run = lambda G: evaluate_model_link_prediction("GraphMixer", model, sampler, get_idx_data_loader(list(range(80)), 40, False),
                                                   NegativeEdgeSampler(d.src_node_ids, d.dst_node_ids, seed=0), eval_data, torch.nn.BCELoss(),
                                                   num_neighbors=cfg["K"], time_gap=G)[0]
    a, b, a2 = run(2000), run(1), run(2000)
    assert a == a2 and len(a) == 2 and a != b
