"""dyglib_amd.TCL as a drop-in in the reference's evaluation loop, written out by hand here (evaluate_models_utils.py:36-150: the fused
evaluate_model_link_prediction does not take "TCL" yet), on an MI355X against the reference's own run (tests/golden/eval_tcl.npz,
tools/make_golden_tcl.py): the negative draws bit-equal, the per-batch loss / AUC / AP within the bars of
tests/test_evaluate.py::test_evaluation_loop_matches_reference (1e-5 / 2e-3 / 1e-2)."""
import numpy as np
import pytest

from tests import golden_cases as gc
from tests import tcl_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_hand_written_evaluation_loop_matches_reference():
    import torch
    from dyglib_amd import TCL, Data, MergeLayer, NegativeEdgeSampler, get_idx_data_loader, get_link_prediction_metrics, get_neighbor_sampler
    c = tc.build_eval_case()
    cfg = c["tcl_cfg"]
    g = gc.load_golden("eval_tcl")
    d = c["data"]
    sampler = get_neighbor_sampler(d, cfg["strategy"], seed=cfg["sampler_seed"], device=DEV)
    bb = TCL(c["node_feat"], c["edge_feat"], sampler, cfg["time_feat_dim"], num_layers=cfg["layers"], num_heads=cfg["heads"], num_depths=cfg["K"] + 1,
             dropout=0.1, device=DEV)
    bb.load_state_dict({k: torch.from_numpy(v) for k, v in c["tcl_params"].items()}, strict=True)
    merge = MergeLayer(172, 172, 172, 1)
    merge.load_state_dict({k: torch.from_numpy(v) for k, v in c["mparams"].items()}, strict=True)
    model = torch.nn.Sequential(bb, merge).to(DEV)
    first, last = gc.eval_indices(d.num_interactions)
    sl = slice(first, last)
    ev = Data(d.src_node_ids[sl], d.dst_node_ids[sl], d.node_interact_times[sl], d.edge_ids[sl], d.labels[sl])
    loader = get_idx_data_loader(list(range(last - first)), cfg["batch"], shuffle=False)
    neg = NegativeEdgeSampler(src_node_ids=d.src_node_ids, dst_node_ids=d.dst_node_ids, seed=gc.EVAL_NEG_SEED)
    loss_func = torch.nn.BCELoss()
    neg.reset_random_state()
    model[0].set_neighbor_sampler(sampler)
    model.eval()
    losses, metrics, draws = [], [], []
    with torch.no_grad():
        for idx in loader:
            idx = idx.numpy()
            src, dst, t = ev.src_node_ids[idx], ev.dst_node_ids[idx], ev.node_interact_times[idx]
            _, neg_dst = neg.sample(size=len(src))
            draws.append(neg_dst)
            s_pos, e_dst, s_neg, e_neg = model[0].compute_step_embeddings(src, dst, neg_dst, t, num_neighbors=cfg["K"])
            pos = model[1](input_1=s_pos, input_2=e_dst).squeeze(dim=-1).sigmoid()
            ngt = model[1](input_1=s_neg, input_2=e_neg).squeeze(dim=-1).sigmoid()
            predicts = torch.cat([pos, ngt], dim=0)
            labels = torch.cat([torch.ones_like(pos), torch.zeros_like(ngt)], dim=0)
            losses.append(loss_func(input=predicts, target=labels).item())
            metrics.append(get_link_prediction_metrics(predicts=predicts, labels=labels))
    assert np.array_equal(np.concatenate(draws), g["neg_dst"])
    assert len(losses) == len(g["losses"])
    errs = (np.abs(np.array(losses) - g["losses"]).max(), np.abs(np.array([m["roc_auc"] for m in metrics]) - g["roc_auc"]).max(),
            np.abs(np.array([m["average_precision"] for m in metrics]) - g["average_precision"]).max())
    print(f"tcl evaluation: max |loss err| {errs[0]:.3e}, |auc err| {errs[1]:.3e}, |ap err| {errs[2]:.3e}")
    assert errs[0] <= 1e-5
    assert errs[1] <= 2e-3
    assert errs[2] <= 1e-2
