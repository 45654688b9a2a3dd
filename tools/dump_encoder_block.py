"""What the kernels shared by TCL, CAWN, TGAT and GraphMixer compute, as bits: for an A/B between two builds of the library.

    python tools/dump_encoder_block.py --out FILE.npz
        runs, with fixed seeds on the smallest fixture cases of each backbone (tests/*_cases.py), on cuda:0:
          inf/...   inference outputs of TCL and CAWN through both entry points (compute_src_dst_node_temporal_embeddings and
                    compute_step_embeddings), CAWN at attention_dim 312 (k_encoder_post<5, 2>), 236 (<4, 4>) and 324 (<8, 2>)
          fwd/...   training-forward outputs of TCL, CAWN, GraphMixer and TGAT at dropout 0.1 with _fixed_dropout_seed set
          grad/...  every parameter gradient of those training calls (the fixture loss of tests/golden_cases.py)
    python tools/dump_encoder_block.py --compare A1.npz A2.npz B1.npz B2.npz [A3.npz ...]
        A = two or more runs of the parent build, B = two runs of the build under test.  inf/ and fwd/ must be numpy.array_equal between A
        and B.  The weight-gradient products add with float atomics (gemm.h), so a gradient need not repeat bit for bit on one build: per
        tensor, where A1 == A2 the B runs must equal A1; elsewhere max |B - A1| may not exceed twice max |A1 - A2|.  Two runs sample the
        atomic-order noise once: a tensor that exceeds this bound, and only such a tensor, is held to twice the largest figure over
        the pairs of ALL parent runs given, and is marked.  Prints a markdown table of every figure and exits 1 on a
        violation.

Reads nothing outside the repository."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

P_DROP, SEED = 0.1, (7 << 40) + 20240


def _loss(s, d):
    import torch
    from tests import golden_cases as gc
    G1, G2 = gc.grad_loss_weights(s.shape[0])
    return (s * torch.from_numpy(G1).to(s.device)).sum() + (d * torch.from_numpy(G2).to(d.device)).sum()


def _train(out, tag, m, call):
    """one training call at P_DROP / SEED and its backward -> fwd/<tag>/{src,dst}, grad/<tag>/<parameter>"""
    m.train()
    m.dropout, m._fixed_dropout_seed = P_DROP, SEED
    m.zero_grad(set_to_none=True)
    s, d = call(m)
    _loss(s, d).backward()
    out[f"fwd/{tag}/src"], out[f"fwd/{tag}/dst"] = s.detach().cpu().numpy(), d.detach().cpu().numpy()
    for n, p in m.named_parameters():
        if p.grad is not None:
            out[f"grad/{tag}/{n}"] = p.grad.detach().cpu().numpy()


def _inference(out, tag, m, c, k):
    import torch
    m.eval()
    with torch.no_grad():
        m.set_neighbor_sampler(m.neighbor_sampler)
        pair = m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=k)
        m.set_neighbor_sampler(m.neighbor_sampler)
        step = m.compute_step_embeddings(c["src"], c["dst"], c["neg_dst"], c["times"], num_neighbors=k)
    for i, x in enumerate(pair):
        out[f"inf/{tag}/pair{i}"] = x.cpu().numpy()
    for i, x in enumerate(step):
        out[f"inf/{tag}/step{i}"] = x.cpu().numpy()


def dump() -> dict:
    import torch
    from tests import cawn_edge_cases as ce
    from tests import golden_cases as gc
    from tests import test_cawn_gpu, test_cawn_train_gpu, test_graphmixer_gpu, test_tcl_gpu, test_tgat_train_gpu
    out = {}
    # TCL: one layer, K = 5, d = 172
    name = "gen_k5_l1_h2"
    c, cfg, m = test_tcl_gpu.case_model(name)
    _inference(out, f"tcl/{name}", m, c, cfg["K"])
    m.set_neighbor_sampler(m.neighbor_sampler)
    _train(out, f"tcl/{name}", m, lambda m: m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=cfg["K"]))
    # CAWN: attention_dim 312 (W = 1, k = 5) and 236 (W = 2, k = 4)
    for name in ("gen_w1_k5", "hub_w2_k4"):
        c, cfg, m, _ = test_cawn_gpu.case_model(name)
        _inference(out, f"cawn/{name}", m, c, cfg["k"])
        c, cfg, m = test_cawn_train_gpu._train_case(name, P_DROP, SEED)
        _train(out, f"cawn/{name}", m, lambda m: m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=cfg["k"]))
    # CAWN inference past 320 columns (attention_dim 324), on the sides of the edge-shape case
    c = ce.shape_case("P204_h6")
    r = c["cfg"]
    m = test_cawn_train_gpu.make_model(c["data"], c["node_feat"], c["edge_feat"], c["params"], r["Ft"], r["P"], r["W"], r["heads"]).eval()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(test_cawn_gpu.DEV)
    roots, times, hops = c["sides"]
    with torch.no_grad():
        oa, ob = m._forward((dev(roots), dev(times), [tuple(dev(x) for x in h) for h in hops]), c["pair_a"], c["pair_b"], r["k"])
    out["inf/cawn/P204_h6/a"], out["inf/cawn/P204_h6/b"] = oa.cpu().numpy(), ob.cpu().numpy()
    # GraphMixer and TGAT: training only (their inference paths share nothing with the block)
    name = "gen_k10_g7"
    c, cfg, m = test_graphmixer_gpu.case_model(name)
    _train(out, f"graphmixer/{name}", m,
           lambda m: m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=cfg["K"], time_gap=cfg["G"]))
    name = "tgat_hub_l1_k10"
    c = gc.build_tgat_case(name)
    m = test_tgat_train_gpu._model(c)
    _train(out, f"tgat/{name}", m,
           lambda m: m.compute_src_dst_node_temporal_embeddings(c["src"], c["dst"], c["times"], num_neighbors=c["tgat_cfg"]["num_neighbors"]))
    torch.cuda.synchronize()
    return out


def compare(paths) -> int:
    runs = [dict(np.load(p)) for p in paths]
    a1, a2, b1, b2 = runs[:4]
    extra = runs[4:]                     # further parent runs
    keys = sorted(a1)
    bad = [f"key sets differ: {p}" for p, r in zip(paths[1:], runs[1:]) if sorted(r) != keys]
    diff = lambda x, y: float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()) if x.size else 0.0
    exact = [k for k in keys if not k.startswith("grad/")]
    n_eq = 0
    for k in exact:
        same = all(np.array_equal(a1[k], r[k]) for r in runs[1:])
        n_eq += same
        if not same:
            bad.append(f"{k}: outputs differ (max |B1 - A1| = {diff(b1[k], a1[k]):.3e}, max |A2 - A1| = {diff(a2[k], a1[k]):.3e})")
    print(f"inference and training-forward outputs: {n_eq} of {len(exact)} tensors numpy.array_equal across all runs\n")
    print("| gradient tensor | max abs | parent 2 vs parent 1 |" + (f" largest over the pairs of all {2 + len(extra)} parent runs |" if extra else "")
          + " branch 1 vs parent 1 | branch 2 vs parent 1 | |")
    print("|---|---|---|" + ("---|" if extra else "") + "---|---|---|")
    n_noisy = 0
    for k in keys:
        if not k.startswith("grad/"):
            continue
        par = [a1, a2] + extra
        aa = [diff(a2[k], a1[k])] + ([max(diff(x[k], y[k]) for i, x in enumerate(par) for y in par[:i])] if extra else [])
        e1, e2 = diff(b1[k], a1[k]), diff(b2[k], a1[k])
        if max(aa) == 0.0 and e1 == 0.0 and e2 == 0.0:
            continue
        n_noisy += 1
        bound, note = 2.0 * aa[0], ""                    # the two-run figure; the further runs count only for a tensor that exceeds it
        if max(e1, e2) > bound and extra:
            bound, note = 2.0 * aa[1], "needs the further parent runs"
        print(f"| {k[5:]} | {float(np.abs(a1[k]).max()):.3e} | " + " | ".join(f"{x:.3e}" for x in aa + [e1, e2]) + f" | {note} |")
        if max(e1, e2) > bound:
            bad.append(f"{k}: branch vs parent {max(e1, e2):.3e} > 2 x parent vs parent {bound / 2.0:.3e}")
    n_grad = sum(k.startswith("grad/") for k in keys)
    print(f"\n{n_grad - n_noisy} of {n_grad} gradient tensors are bit-identical across all runs (not listed); {n_noisy} listed above.")
    for line in bad:
        print("VIOLATION:", line)
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs="+")
    args = ap.parse_args()
    if args.compare:
        assert len(args.compare) >= 4, "--compare A1 A2 B1 B2 [A3 ...]"
        sys.exit(compare(args.compare))
    assert args.out, "--out FILE.npz"
    res = dump()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez(args.out, **res)
    print(f"wrote {args.out}: {len(res)} tensors")
