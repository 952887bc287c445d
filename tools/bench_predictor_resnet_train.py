#!/usr/bin/env python
"""ms per training step of ``ChestPredictorTrainStep`` (csrc/predictor_resnet_train.inc: mimic's GroupNorm ResNet-18 heads, one
trunk pass, Dropout 0.2, AdamW + EMA, captured) at mimic192 (R = 192) and mimic224, B = 32 -- against the same step in torch
eager f32 on the same card in the same process (``ChestPredictor.torch_outputs`` with Dropout added + the likelihoods + autograd
+ ``clip_grad_norm_`` + ``torch.optim.AdamW`` + an EMA update), once with the trunk shared and once as the reference runs it
(four trunk passes, one per head).

Method: warm-up steps, then HIP events around STEPS consecutive steps; RUNS runs per path with the paths ALTERNATED run by run;
the median and the spread (min .. max) are printed, the workspace size, and one JSON line with everything.  The goal is "faster
than the four-pass way in every run"; the ratio to the shared-trunk eager step is reported, not gated.  Last, one kernel-trace
run of the captured step alone (a fresh child process under rocprofv3) gives the share of each kernel class.

    python tools/bench_predictor_resnet_train.py [--steps 200] [--warmup 10] [--runs 3] [--batch 32] [--no-trace]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from tools.bench_predictor_resnet import eager_nll, one_run, randomise  # noqa: E402

P_DROPOUT = 0.2
CLASSES = (("wgrad_kernel", "conv weight gradient (f32 MFMA)"), ("wred_kernel", "split-K reduce"), ("conv_", "conv forward / data gradient"),
           ("im2col", "im2col / col2im"), ("col2im", "im2col / col2im"), ("rn_gnp", "GroupNorm parameter gradients"),
           ("rn_gn", "GroupNorm statistics / apply / backward"), ("rn_drop", "Dropout"), ("rn_scale", "Dropout"), ("rn_pool", "max pool"),
           ("rn_tail", "heads"), ("wprep", "weight images"), ("adamw", "optimiser tail"), ("sumsq", "optimiser tail"),
           ("clip_decide", "optimiser tail"), ("step_commit", "optimiser tail"))


class EagerStep:
    """The reference's sup_epoch step in torch eager f32 on a copy of the predictor: Dropout through ``F.dropout`` after every
    ``relu(bn1)`` (``torch_features`` has none: it is patched in here), AdamW under a constant lr, clip, EMA."""

    def __init__(self, pred, obs, shared):
        import copy

        self.pred, self.obs, self.shared = copy.deepcopy(pred).cuda(), obs, shared
        self.params = [p for p in self.pred.parameters()]
        for p in self.params:
            p.requires_grad_(True)
        self.opt = torch.optim.AdamW(self.params, lr=1e-4, weight_decay=0.1, betas=(0.9, 0.999), eps=1e-8)
        self.ema = [p.detach().clone() for p in self.params]
        self._patch()

    def _patch(self):
        from causal_gen_amd.predictor_resnet import _blocks

        pred = self.pred

        def features(x):
            t = pred.encoder_s.resnet
            cv = lambda h, m: F.conv2d(h, m.weight, None, m.stride, m.padding)
            h = F.max_pool2d(F.relu(pred._gn(cv(x, t[0]), t[1])), 3, 2, 1)
            for b in _blocks(t):
                idn = h if b.downsample is None else pred._gn(cv(h, b.downsample[0]), b.downsample[1])
                o = F.dropout(F.relu(pred._gn(cv(h, b.conv1), b.bn1)), P_DROPOUT, True)
                h = F.relu(pred._gn(cv(o, b.conv2), b.bn2) + idn)
            return h.mean(dim=(2, 3))

        pred.torch_features = features

    def __call__(self):
        B = self.obs["x"].shape[0]
        self.opt.zero_grad(set_to_none=True)
        loss = eager_nll(self.pred, self.obs, self.obs["x"], self.shared) / B
        loss.backward()
        torch.nn.utils.clip_grad_norm_(self.params, 200.0)
        self.opt.step()
        with torch.no_grad():
            torch._foreach_lerp_(self.ema, [p.detach() for p in self.params], 1 - 0.999)
        return loss


def make(R, B):
    from causal_gen_amd.predictor_resnet import ChestPredictor

    pred = randomise(ChestPredictor(SimpleNamespace(input_channels=1, input_res=R, std_fixed=0.0)), 1).cuda()
    g = torch.Generator().manual_seed(2)
    obs = {"x": torch.rand(B, 1, R, R, generator=g) * 2 - 1, "sex": torch.randint(0, 2, (B, 1), generator=g).float(),
           "race": F.one_hot(torch.randint(0, 3, (B,), generator=g), 3).float(),
           "finding": torch.randint(0, 2, (B, 1), generator=g).float(), "age": torch.rand(B, 1, generator=g) * 2 - 1}
    return pred, {k: v.cuda().contiguous() for k, v in obs.items()}


def kernel_shares(res, batch):
    """{class: share of the kernel time} of the captured step, from a kernel trace of a child process of its own."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "t", "--output-format", "csv", "--", sys.executable,
               os.path.abspath(__file__), "--profile", "20", "--res", str(res), "--batch", str(batch)]
        try:
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        except (OSError, subprocess.SubprocessError) as e:
            return {"error": f"kernel trace failed: {e}"}
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"error": "the kernel trace left no kernel_stats.csv"}
        total, by = 0.0, {}
        for row in csv.DictReader(open(files[0])):
            name, ns = row.get("Name", ""), float(row.get("TotalDurationNs", 0) or 0)
            label = next((lab for key, lab in CLASSES if key in name), "other (torch element-wise, copies)")
            by[label] = by.get(label, 0.0) + ns
            total += ns
        return {k: v / total for k, v in sorted(by.items(), key=lambda kv: -kv[1])} if total else {"error": "empty trace"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--res", type=int, nargs="*", default=[192, 224])
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--profile", type=int, default=0, help="only run the captured step this many times (for a kernel trace)")
    a = ap.parse_args()
    from causal_gen_amd import _lib
    from causal_gen_amd.predictor_resnet_train import ChestPredictorTrainStep

    _lib.require_gpu()
    rows, B = [], a.batch
    for R in a.res:
        pred, obs = make(R, B)
        ts = ChestPredictorTrainStep(pred, p_dropout=P_DROPOUT)
        for _ in range(3):  # the eager first step, the capture, a replay
            ts.step(**obs)
        ent = next(iter(ts._statics.values()))
        graph = next(iter(ts._graphs.values()))
        if a.profile:
            for _ in range(a.profile):
                graph.replay()
            torch.cuda.synchronize()
            continue
        paths = {"hip_step_graph": graph.replay, "hip_step_with_input_copies": lambda: ts.step(**obs),
                 "torch_shared_step": EagerStep(pred, obs, True), "torch_four_pass_step": EagerStep(pred, obs, False)}
        for fn in paths.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in paths}
        for _ in range(a.runs):  # alternated: one run of every path, then the next round
            for k, fn in paths.items():
                times[k].append(one_run(fn, a.steps))
        need, ev = _lib.i64(0), _lib.i64(0)
        import ctypes

        ts.lib.resnet_train_workspace(B, R, ctypes.byref(need))
        ts.lib.resnet_workspace(B, R, ctypes.byref(ev))
        row = dict(res=R, B=B, workspace_mib=need.value * 4 / 2 ** 20, eval_workspace_mib=ev.value * 4 / 2 ** 20, loss=float(ts.res[0]),
                   opt_steps=ts.stats()["opt_steps"], n_skipped=ts.stats()["n_skipped"])
        assert ent["ws"].numel() == need.value
        print(f"mimic{R} B={B}: workspace {row['workspace_mib']:.1f} MiB (eval {row['eval_workspace_mib']:.1f} MiB); loss {row['loss']:.4f} "
              f"after {row['opt_steps']} steps, {row['n_skipped']} skipped")
        for k, v in times.items():
            v = sorted(v)
            row[k] = dict(ms=v[len(v) // 2], min=v[0], max=v[-1])
            print(f"  {k:28s} {v[len(v) // 2]:9.4f} ms ({v[0]:.4f} .. {v[-1]:.4f})")
        ok = max(row["hip_step_graph"]["max"], row["hip_step_with_input_copies"]["max"]) < row["torch_four_pass_step"]["min"]
        row["faster_than_four_pass_eager_in_every_run"] = bool(ok)
        row["ratio_to_shared_eager"] = row["hip_step_graph"]["ms"] / row["torch_shared_step"]["ms"]
        print(f"  faster than the four-pass eager step in every run: {ok}; captured step / shared-trunk eager step: {row['ratio_to_shared_eager']:.3f}")
        if not a.no_trace:
            row["kernel_shares"] = kernel_shares(R, B)
            for k, v in row["kernel_shares"].items():
                print(f"  {k:44s} {v if isinstance(v, str) else f'{100 * v:5.1f} %'}")
        rows.append(row)
    if not a.profile:
        print(json.dumps(dict(bench="predictor_resnet_train", steps=a.steps, warmup=a.warmup, runs=a.runs, rows=rows)))


if __name__ == "__main__":
    main()
