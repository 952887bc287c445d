#!/usr/bin/env python
"""ms per counterfactual-parents call: ``PgmCounterfactual.run`` inside a captured graph (csrc/pgm_cf.hip, one launch) against the
host path it replaces -- ``pgm.counterfactual`` + ``dscm.vae_preprocess`` in torch eager on the same card, in the same run.
FlowPGM (do(age): both volumes are re-predicted) and MorphoMNISTPGM (do(thickness)) at B = 32 and B = 1024.

Method: warm-up calls, then HIP events around REPLAYS consecutive calls, three runs per cell; the median and the spread
(min .. max) of the three are printed, and one JSON line with everything.  No target is fixed: the claim to check is "below eager
in the same run", not a ratio.

    python tools/bench_pgm_cf.py [--replays 200] [--warmup 30] [--runs 3]
"""
import argparse
import copy
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.bench_pgm_train import make, timed  # noqa: E402

ARGS = {"flow": SimpleNamespace(parents_x=["mri_seq", "brain_volume", "ventricle_volume", "sex"], dataset="ukbb192", input_res=192),
        "morpho": SimpleNamespace(parents_x=["thickness", "intensity", "digit"], dataset="morphomnist", input_res=32)}
DO = {"flow": "age", "morpho": "thickness"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    from causal_gen_amd import dscm
    from causal_gen_amd.pgm_cf import PgmCounterfactual
    from causal_gen_amd.pgm_train import default_columns

    rows = []
    for kind in ("flow", "morpho"):
        for B in (32, 1024):
            m = make(kind)
            args, var = ARGS[kind], DO[kind]
            obs = {k: v.cuda() for k, v in m.sample(B, generator=torch.Generator().manual_seed(2)).items()}
            perm = torch.randperm(B, generator=torch.Generator().manual_seed(3)).cuda()
            cols, ncol = default_columns(m)
            table = torch.cat([obs[k] for k in m.variables], 1).contiguous()
            assert table.shape[1] == ncol
            cf = PgmCounterfactual(copy.deepcopy(m), args)
            cf.run(table, None, table, perm, do_vars=[var])
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                cf.run(table, None, table, perm, do_vars=[var])
            hip = timed(graph.replay, a.warmup, a.replays, a.runs)
            host = copy.deepcopy(m).cuda()

            @torch.no_grad()
            def eager():
                do = {var: obs[var][perm]}
                cf_pa = host.counterfactual(obs=obs, intervention=do, num_particles=1)
                return dscm.vae_preprocess(args, {k: v.clone() for k, v in obs.items()}), dscm.vae_preprocess(args, {k: v.clone() for k, v in cf_pa.items()})

            eag = timed(eager, a.warmup, a.replays, a.runs)
            mid = len(hip) // 2
            rows.append(dict(pgm=kind, B=B, do=var, hip_ms=hip[mid], hip_min=hip[0], hip_max=hip[-1], eager_ms=eag[mid], eager_min=eag[0],
                             eager_max=eag[-1], below_eager=hip[-1] < eag[0]))
            print(f"{kind:7s} B={B:5d} do({var})  PgmCounterfactual {hip[mid]:.4f} ms ({hip[0]:.4f} .. {hip[-1]:.4f})   "
                  f"torch eager {eag[mid]:.4f} ms ({eag[0]:.4f} .. {eag[-1]:.4f})   below eager in every run: {hip[-1] < eag[0]}")
    print(json.dumps(dict(bench="pgm_cf", replays=a.replays, warmup=a.warmup, runs=a.runs, rows=rows)))


if __name__ == "__main__":
    main()
