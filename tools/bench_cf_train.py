#!/usr/bin/env python
"""ms per counterfactual fine-tuning step: CfTrainStep (captured: one hipGraph per step) against the host composition a user had
before it -- ``DSCM.forward`` under autograd (its NaN check and ``.item()`` syncs included) + ``backward`` + ``clip_grad_norm_`` + two
``torch.optim.AdamW`` (the multiplier's with ``maximize=True``) + the clamp + a Python EMA loop -- on the same card, in the same run,
the two paths alternated.  morphomnist and ukbb192 at B = 32, f32 engine, random weights (the recipe of oracle/fullsize_recipe),
fixed counterfactual parents on both sides (the parent SCM is outside both timings).  ``--presets mimic192`` adds mimic's cell: the
mimic192 HVAE with ``ChestPredictor`` (constructed directly: ``make_predictor`` keeps its answer for mimic) on ``ChestPGM``'s variables.

Method: warm-up steps, then HIP events around STEPS consecutive steps, RUNS times per path with the paths taking turns; the
median and the spread (min .. max) are printed, with ABOUT how many kernels a replayed step has (the engine's launch counter over
the eager first step plus the step's own library launches: torch's few small kernels -- copies, the scalar heads -- are not counted),
and one JSON line stamped with the tree hash.  The claim to check is "below the host composition in every run", not a ratio.

    python tools/bench_cf_train.py [--steps 20] [--warmup 5] [--runs 3] [--presets morphomnist,ukbb192[,mimic192]]
"""
import argparse
import copy
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

B = 32
LR, LR_LAG, EMA_RATE = 1e-4, 1e-2, 0.999


class FixedPGM(torch.nn.Module):
    """``pgm.counterfactual`` with a fixed answer: the parent SCM is not what is measured."""

    def __init__(self, cf):
        super().__init__()
        self.cf = cf

    def counterfactual(self, obs, intervention, num_particles=1):
        return dict(self.cf)


def variables(preset, g):
    if preset == "morphomnist":
        oh = torch.nn.functional.one_hot(torch.randint(0, 10, (B,), generator=g), 10).float()
        return {"thickness": torch.rand(B, 1, generator=g) * 1.6 - 0.8, "intensity": torch.rand(B, 1, generator=g) * 1.6 - 0.8, "digit": oh}
    r = lambda: torch.rand(B, 1, generator=g) * 1.6 - 0.8  # noqa: E731
    b = lambda: (torch.rand(B, 1, generator=g) < 0.5).float()  # noqa: E731
    if preset == "mimic192":
        return {"age": r(), "race": torch.nn.functional.one_hot(torch.randint(0, 3, (B,), generator=g), 3).float(), "sex": b(), "finding": b()}
    return {"mri_seq": b(), "brain_volume": r(), "ventricle_volume": r(), "age": r(), "sex": b()}


def build(preset):
    from causal_gen_amd import dscm, predictor, vae
    from causal_gen_amd.hps import setup_hparams
    from oracle import fullsize_recipe as R

    hp = setup_hparams(preset, cond_prior=False)
    torch.manual_seed(7)
    m = vae.HVAE(hp)
    m.apply(R.init_bias)
    R.perturb(m)
    m.compute_dtype = "f32"
    x, _ = R.inputs(hp, B)
    g = torch.Generator().manual_seed(3)
    obs, cf = variables(preset, g), variables(preset, g)
    parents = list(obs) if preset in ("morphomnist", "mimic192") else ["mri_seq", "brain_volume", "ventricle_volume", "sex"]
    assert sum(v.shape[1] for k, v in obs.items() if k in parents) == hp.context_dim, (preset, hp.context_dim)
    args = SimpleNamespace(**{**vars(hp), "parents_x": parents, "dataset": preset, "lmbda_init": 0.8, "elbo_constraint": 2.0, "damping": 10.0,
                              "grad_skip": 1e9, "ema_rate": EMA_RATE})
    pargs = SimpleNamespace(dataset=preset, input_channels=hp.input_channels, input_res=hp.input_res, std_fixed=0.0)
    if preset == "mimic192":
        from causal_gen_amd.predictor_resnet import ChestPredictor

        pred = ChestPredictor(pargs)
    else:
        pred = predictor.make_predictor(pargs)
    cf = {k: v.cuda() for k, v in cf.items()}
    model = dscm.DSCM(args, FixedPGM(cf), pred, m.eval()).cuda()
    for p in m.parameters():
        p.requires_grad_(True)
    batch = {"x": x.cuda(), **{k: v.cuda() for k, v in obs.items()}}
    return model, args, batch, cf


def host_step_fn(model, args, batch):
    """train_cf.py:159-177 as a user composes it today on this backend"""
    from causal_gen_amd.predictor import AnticausalELBO

    elbo_fn = AnticausalELBO()
    params = [p for n, p in model.named_parameters() if n != "lmbda" and p.requires_grad]
    opt = torch.optim.AdamW(params, lr=LR, weight_decay=args.wd, betas=tuple(args.betas))
    lag = torch.optim.AdamW([model.lmbda], lr=LR_LAG, betas=tuple(args.betas), weight_decay=0, maximize=True)
    ema = [p.detach().clone() for p in params + [model.lmbda]]

    def step():
        opt.zero_grad(set_to_none=True)
        lag.zero_grad(set_to_none=True)
        out = model(batch, {"thickness": None}, elbo_fn, cf_particles=1)  # (FixedPGM answers whatever the intervention is)
        if torch.isnan(out["loss"]):
            return
        out["loss"].sum().backward()
        norm = torch.nn.utils.clip_grad_norm_(params + [model.lmbda], args.grad_clip)
        if norm < args.grad_skip:
            opt.step()
            lag.step()
            model.lmbda.data.clamp_(min=0)
            with torch.no_grad():
                for e, p in zip(ema, params + [model.lmbda]):
                    e.sub_((e - p) * (1.0 - EMA_RATE))
        float(out["loss"].detach())  # the per-step .item() of train_cf.py:205

    return step


def device_step_fn(model, args, batch, cf):
    from causal_gen_amd.cf_train import CfTrainStep
    from causal_gen_amd.dscm import vae_preprocess

    step = CfTrainStep(model, args, lr=LR, lr_lagrange=LR_LAG, use_graph=True)
    pa = vae_preprocess(args, {k: v.clone() for k, v in batch.items() if k != "x"})
    cf_pa = vae_preprocess(args, {k: v.clone() for k, v in cf.items()})
    x = batch["x"]
    eng = step.eng
    before = eng.launches
    step.step(x, pa, cf_pa, cf)  # eager, then captured: the launch counter saw the step twice
    tail = 2 + len(step.ranges) + 2
    # the CNN heads are one launch each way; ChestPredictor's two plans (csrc/predictor_resnet.inc rn_forward / rn_backward, counted
    # launch by launch with one kernel per conv) are 84 forward with the sum of the terms and 90 backward
    pred = 84 + 90 if type(step.pred).__name__ == "ChestPredictor" else 2
    kernels = (eng.launches - before) // 2 + pred + 2 + 1 + tail  # engine passes + predictor fwd / bwd + non-finite x2 + Lagrangian + tail
    return (lambda: step.step(x, pa, cf_pa, cf)), step, kernels


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    from tree_sha import tree_sha

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--presets", default="morphomnist,ukbb192")
    a = ap.parse_args()
    res = {"code_tree_sha": tree_sha(ROOT), "B": B, "steps": a.steps, "runs": a.runs, "dtype": "f32", "cells": {}}
    for preset in a.presets.split(","):
        model, args, batch, cf = build(preset)
        host_model = copy.deepcopy(model)  # (own weights and engine: the two paths do not train each other's model)
        host = host_step_fn(host_model, args, batch)
        dev, step, kernels = device_step_fn(model, args, batch, cf)
        for _ in range(a.warmup):
            host()
            dev()
        torch.cuda.synchronize()
        th, td = [], []
        for _ in range(a.runs):  # alternated: both see the same clocks and the same neighbours
            th.append(timed(host, a.steps))
            td.append(timed(dev, a.steps))
        st = step.stats()
        cell = {"host_ms": sorted(th), "device_ms": sorted(td), "kernels_per_step_about": kernels, "opt_steps": st["opt_steps"], "n_bad": st["n_bad"],
                "below_in_every_run": all(d < h for d, h in zip(td, th)) and max(td) < min(th)}
        res["cells"][preset] = cell
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        print(f"{preset:12s} B={B} f32  host composition {med(th):8.2f} ms ({min(th):.2f} .. {max(th):.2f})   CfTrainStep {med(td):8.2f} ms "
              f"({min(td):.2f} .. {max(td):.2f})   about {kernels} kernels / step   {'below in every run' if cell['below_in_every_run'] else 'MISSED'}")
        del model, host_model, step, dev, host
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
