#!/usr/bin/env python
"""ms per training step of the parent SCM: PgmTrainStep (captured: csrc/pgm.hip + the optimiser tail, one hipGraph) against the
only alternative a user of the parent commit has -- the host module's ``nll`` + ``torch.optim.AdamW`` + LambdaLR + clip + EMA in
torch eager on the same card, in the same run.  FlowPGM and MorphoMNISTPGM at B = 32 and B = 1024.

Method: warm-up steps, then HIP events around REPLAYS consecutive steps, three runs per cell; the median and the spread
(min .. max) of the three are printed, and one JSON line with everything.  The claim to check is "below eager in the same run",
not a ratio.

    python tools/bench_pgm_train.py [--replays 200] [--warmup 30] [--runs 3]
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

HP = dict(lr=1e-3, wd=0.1, betas=(0.9, 0.999), eps=1e-8, grad_clip=200.0, lr_warmup_steps=1, ema_rate=0.999, ema_update_after=100)


def make(kind):
    from causal_gen_amd import pgm

    torch.manual_seed(0)
    m = {"flow": pgm.FlowPGM, "morpho": pgm.MorphoMNISTPGM}[kind](SimpleNamespace())
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g))
    return m


def timed(fn, warmup, replays, runs):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(replays):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / replays)
    return sorted(out)


def eager_step_fn(m, obs):
    """sup_epoch's step in torch eager on the device: nll, backward, clip, AdamW under LambdaLR, the project's EMA rule"""
    from oracle import train_ref

    m = copy.deepcopy(m).cuda()
    params = list(m.parameters())
    ema = [p.detach().clone() for p in params]
    opt = torch.optim.AdamW(params, lr=HP["lr"], weight_decay=HP["wd"], betas=HP["betas"], eps=HP["eps"])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, train_ref.linear_warmup(HP["lr_warmup_steps"]))
    t = [0]

    def step():
        opt.zero_grad(set_to_none=True)
        loss = m.nll(obs)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, HP["grad_clip"])
        opt.step()
        sched.step()
        d = train_ref.ema_decay(t[0], HP["ema_rate"], HP["ema_update_after"])
        with torch.no_grad():
            if d is None:
                torch._foreach_copy_(ema, params)
            else:
                torch._foreach_lerp_(ema, params, 1.0 - d)
        t[0] += 1

    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    from causal_gen_amd.pgm_train import PgmTrainStep

    rows = []
    for kind in ("flow", "morpho"):
        for B in (32, 1024):
            m = make(kind)
            obs = {k: v.cuda() for k, v in m.sample(B, generator=torch.Generator().manual_seed(2)).items()}
            ts = PgmTrainStep(copy.deepcopy(m), **HP)
            hip = timed(lambda: ts.step(**obs), a.warmup, a.replays, a.runs)
            assert ts.stats()["n_skipped"] == 0
            eag = timed(eager_step_fn(m, obs), a.warmup, a.replays, a.runs)
            mid = len(hip) // 2
            rows.append(dict(pgm=kind, B=B, hip_ms=hip[mid], hip_min=hip[0], hip_max=hip[-1], eager_ms=eag[mid], eager_min=eag[0],
                             eager_max=eag[-1], below_eager=hip[-1] < eag[0]))
            print(f"{kind:7s} B={B:5d}  PgmTrainStep {hip[mid]:.4f} ms ({hip[0]:.4f} .. {hip[-1]:.4f})   "
                  f"torch eager {eag[mid]:.4f} ms ({eag[0]:.4f} .. {eag[-1]:.4f})   below eager in every run: {hip[-1] < eag[0]}")
    print(json.dumps(dict(bench="pgm_train", replays=a.replays, warmup=a.warmup, runs=a.runs, rows=rows)))


if __name__ == "__main__":
    main()
