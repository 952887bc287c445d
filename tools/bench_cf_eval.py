#!/usr/bin/env python3
"""Cost of counterfactual evaluation next to the counterfactual loop it measures:
    python tools/bench_cf_eval.py [--config ukbb192] [--dtype f32] [--batch 32] [--k 6] [--rounds 5] [--auc-rows 65536]
Legs, interleaved round by round (medians reported, milliseconds per batch):
  cf_graph        one GraphedCounterfactual replay (the loop alone)
  cf_graph_eval   the same + predictor forward + one cgen_metric_accum launch + one cgen_image_dist call
  eval_k          CfEvaluator.effectiveness with K interventions (one abduction, K replays, K predictor / metric launches)
  cf_k            K independent eager dscm.counterfactual calls (K abductions) -- what eval_k's shared abduction saves
and, once, cgen_rocauc alone at --auc-rows rows.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="ukbb192", choices=["ukbb192", "morphomnist"])
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--auc-rows", type=int, default=65536)
    a = ap.parse_args()
    from causal_gen_amd import _lib, cf_eval, dscm, pgm, predictor

    dev = torch.device("cuda", 0)
    m, hp = bench.build_model(a.config, a.dtype)
    m = m.to(dev).eval()
    if not hp.dataset:
        hp.dataset = a.config
    pargs = SimpleNamespace(dataset=hp.dataset, input_channels=hp.input_channels, input_res=hp.input_res, std_fixed=0.0)
    scm = (pgm.FlowPGM(pargs) if "ukbb" in a.config else pgm.MorphoMNISTPGM(pargs)).to(dev)
    pred = predictor.make_predictor(pargs).to(dev)
    B = a.batch
    pa = scm.sample(B, torch.Generator().manual_seed(1))
    x, _ = bench.synth_batch(a.config, hp, B, dev, seed=100)
    obs = dict(pa, x=x)
    order = list(scm.variables)
    dos = {}
    for i in range(a.k):  # one intervention per DAG variable, then permutations of further shifts (train_cf.py:489-497)
        k = order[i % len(order)]
        dos["do(%s)#%d" % (k, i)] = {k: pa[k].roll(1 + i // len(order), 0)}
    ev = cf_eval.CfEvaluator(m, scm, pred, hp, capacity=a.auc_rows)
    pre, pre_cf = ev._pre(pa), ev._pre(scm.counterfactual(obs=pa, intervention=next(iter(dos.values()))))
    graphed = dscm.GraphedCounterfactual(m)
    acc = cf_eval.MetricAccumulator(ev.specs, a.auc_rows, dev)
    dacc = torch.zeros(3, dtype=torch.float64, device=dev)

    def cf_graph():
        return graphed(x, pre, pre_cf)

    def cf_graph_eval():
        cf_x = graphed(x, pre, pre_cf)
        acc.update_from(pred, x=cf_x, **pa)
        cf_eval.image_distance(x, cf_x, dacc)

    def eval_k():
        ev.effectiveness(obs, dos)

    def cf_k():
        for do in dos.values():
            dscm.counterfactual(m, x, pre, ev._pre(scm.counterfactual(obs=pa, intervention=do)))

    legs = {"cf_graph": cf_graph, "cf_graph_eval": cf_graph_eval, "eval_k": eval_k, "cf_k": cf_k}
    for fn in legs.values():  # warm-up: arena, tables, graph capture, workspaces
        fn()
        fn()
    times = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            times[k].append(timed(fn, a.reps))
    out = {"config": a.config, "dtype": a.dtype, "batch": B, "k": a.k, "rounds": a.rounds, "reps": a.reps,
           "ms_median": {k: statistics.median(v) for k, v in times.items()}, "ms_min": {k: min(v) for k, v in times.items()},
           "ms_max": {k: max(v) for k, v in times.items()}}
    med = out["ms_median"]
    out["eval_overhead_ms"] = med["cf_graph_eval"] - med["cf_graph"]
    out["eval_k_over_cf_k"] = med["eval_k"] / med["cf_k"]

    # cgen_rocauc alone: a full score buffer, binary
    lib = _lib.require_gpu()
    n = a.auc_rows
    g = torch.Generator().manual_seed(2)
    s, lab = torch.rand(n, 1, generator=g).to(dev), (torch.rand(n, 1, generator=g) < 0.4).float().to(dev)
    cnt = torch.tensor([n], dtype=torch.int64, device=dev)
    auc = torch.zeros(1, dtype=torch.float64, device=dev)
    ws = torch.zeros(4, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    run = lambda: lib.rocauc(s.data_ptr(), lab.data_ptr(), cnt.data_ptr(), n, 1, 1, auc.data_ptr(), ws.data_ptr(), st)
    run()
    t = [timed(run, 5) for _ in range(a.rounds)]
    out["rocauc"] = {"rows": n, "ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t), "auc": float(auc.item())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
