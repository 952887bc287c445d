#!/usr/bin/env python
"""ms per call of ``ChestPredictor`` (csrc/predictor_resnet.inc: mimic's GroupNorm ResNet-18 heads, one trunk pass) at
mimic192 (R = 192) and mimic224, B = 32: the forward alone (``nll_terms``'s plan) and forward + input gradient, eager and
inside a captured graph -- against the same network in torch eager f32 on the same card in the same process
(``ChestPredictor.torch_outputs`` + the likelihoods + ``autograd.grad`` w.r.t. x), once as the reference runs it (four trunk
passes, one per head) and once with the trunk shared.

Method: warm-up calls, then HIP events around REPLAYS consecutive calls; RUNS runs per path with the paths ALTERNATED run by
run; the median and the spread (min .. max) are printed, and one JSON line with everything, the workspace size included.
No target is fixed: the claim to check is "no slower than the shared-trunk eager baseline in every run".

    python tools/bench_predictor_resnet.py [--replays 200] [--warmup 10] [--runs 3] [--batch 32]
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_predictor_resnet.py --profile 20 --res 224   (the captured step alone)
"""
import argparse
import ctypes
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def randomise(pred, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in pred.named_parameters():
            n = torch.randn(p.shape, generator=g)
            if p.dim() == 4:
                p.copy_(n * (2.0 / (p.shape[1] * p.shape[2] * p.shape[3])) ** 0.5)
            elif ".fc." in name:
                p.copy_(n / 512 ** 0.5)
            else:
                p.copy_((1.0 if name.endswith("weight") else 0.0) + 0.3 * n)
    return pred


def eager_nll(pred, obs, x, shared):
    """flow_pgm.py:659-689 in torch eager: the four heads' likelihoods through torch.distributions."""
    import torch.distributions as D

    o = pred.torch_outputs(x, obs["finding"], shared=shared)
    loc, ls = o["age"].chunk(2, dim=-1)
    lp = (D.Bernoulli(probs=torch.sigmoid(o["sex"])).log_prob(obs["sex"]).sum()
          + D.OneHotCategorical(probs=F.softmax(o["race"], dim=-1)).log_prob(obs["race"]).sum()
          + D.Bernoulli(probs=torch.sigmoid(o["finding"])).log_prob(obs["finding"]).sum()
          + D.Normal(loc, pred.f(ls)).log_prob(obs["age"]).sum())
    return -lp


def one_run(fn, replays):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / replays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--res", type=int, nargs="*", default=[192, 224])
    ap.add_argument("--profile", type=int, default=0, help="only replay the captured forward + backward this many times (for a kernel trace)")
    a = ap.parse_args()
    from causal_gen_amd import _lib, step_tail
    from causal_gen_amd.predictor_resnet import ChestPredictor

    lib = _lib.require_gpu()
    rows, B = [], a.batch
    for R in a.res:
        pred = randomise(ChestPredictor(SimpleNamespace(input_channels=1, input_res=R, std_fixed=0.0)), 1).cuda()
        g = torch.Generator().manual_seed(2)
        obs = {"x": torch.rand(B, 1, R, R, generator=g) * 2 - 1, "sex": torch.randint(0, 2, (B, 1), generator=g).float(),
               "race": F.one_hot(torch.randint(0, 3, (B,), generator=g), 3).float(),
               "finding": torch.randint(0, 2, (B, 1), generator=g).float(), "age": torch.rand(B, 1, generator=g) * 2 - 1}
        obs = {k: v.cuda().contiguous() for k, v in obs.items()}
        x = obs["x"]
        need = _lib.i64(0)
        lib.resnet_workspace(B, R, ctypes.byref(need))
        run = pred._run(x, obs, need_obs=True)
        terms, loss, dx = torch.empty(B, 4, device="cuda"), torch.empty(1, device="cuda"), torch.empty_like(x)
        coef = torch.ones(1, device="cuda")

        def hip_fwd():
            pred._fwd(run, terms, None, loss)

        def hip_both():
            pred._fwd(run, terms, None, loss)
            pred._bwd(run, coef, dx)

        def base(shared, grad):
            def fn():
                if not grad:
                    with torch.no_grad():
                        return eager_nll(pred, obs, x, shared)
                xg = x.detach().requires_grad_(True)
                return torch.autograd.grad(eager_nll(pred, obs, xg, shared), xg)[0]
            return fn

        hip_both()  # the eager run of the same launches, then the captures
        g_fwd, _ = step_tail.capture(hip_fwd)
        g_both, _ = step_tail.capture(hip_both)
        if a.profile:
            for _ in range(a.profile):
                g_both.replay()
            torch.cuda.synchronize()
            continue
        # same numbers on the inputs that are timed: loss and gradient against the eager baseline
        ref_loss = float(base(True, False)())
        ref_gx = base(True, True)()
        g_both.replay()
        torch.cuda.synchronize()
        loss_err = abs(float(loss) - ref_loss) / max(1.0, abs(ref_loss))
        grad_err = float((dx - ref_gx).abs().max() / ref_gx.abs().max())
        # per image (each image's gradient is its own): a ReLU input within rounding of zero that the two f32 computations put on
        # different sides moves that image's whole gradient by ~1e-2 (LABNOTES 29.1); the others agree to rounding
        per_img = ((dx - ref_gx).flatten(1).abs().amax(1) / ref_gx.flatten(1).abs().amax(1)).tolist()
        paths = {"hip_fwd_eager": hip_fwd, "hip_fwd_graph": g_fwd.replay, "hip_fwd_bwd_eager": hip_both, "hip_fwd_bwd_graph": g_both.replay,
                 "torch_shared_fwd": base(True, False), "torch_shared_fwd_bwd": base(True, True),
                 "torch_four_pass_fwd": base(False, False), "torch_four_pass_fwd_bwd": base(False, True)}
        for fn in paths.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in paths}
        for _ in range(a.runs):  # alternated: one run of every path, then the next round
            for k, fn in paths.items():
                times[k].append(one_run(fn, a.replays))
        row = dict(res=R, B=B, workspace_mib=need.value * 4 / 2 ** 20, loss_rel_err_vs_torch_f32=loss_err, grad_rel_err_vs_torch_f32=grad_err,
                   grad_rel_err_per_image_median=sorted(per_img)[len(per_img) // 2], images_above_1e_4=sum(e > 1e-4 for e in per_img))
        print(f"mimic{R} B={B}: workspace {row['workspace_mib']:.1f} MiB; against torch f32 on these inputs: loss {loss_err:.2e}, input gradient {grad_err:.2e} of its max "
              f"(per image: median {row['grad_rel_err_per_image_median']:.2e}, {row['images_above_1e_4']} of {B} above 1e-4)")
        for k, v in times.items():
            v = sorted(v)
            row[k] = dict(ms=v[len(v) // 2], min=v[0], max=v[-1])
            print(f"  {k:26s} {v[len(v) // 2]:9.4f} ms ({v[0]:.4f} .. {v[-1]:.4f})")
        for way in ("fwd", "fwd_bwd"):
            ok = max(row[f"hip_{way}_graph"]["max"], row[f"hip_{way}_eager"]["max"]) <= row[f"torch_shared_{way}"]["min"]
            row[f"{way}_no_slower_than_shared_eager_in_every_run"] = bool(ok)
            print(f"  {way}: no slower than the shared-trunk eager baseline in every run: {ok}")
        rows.append(row)
    print(json.dumps(dict(bench="predictor_resnet", replays=a.replays, warmup=a.warmup, runs=a.runs, rows=rows)))


if __name__ == "__main__":
    main()
