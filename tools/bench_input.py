#!/usr/bin/env python3
"""Input pipeline on the device (causal_gen_amd.data, cgen_batch_augment) next to the paths it replaces, per preset, on a synthetic
resident data set of the preset's shape.  One JSON line per preset:

  kernel_us / kernel_gbs   cgen_batch_augment into the engine's input tensor (pixel stride 8, compute dtype), bytes = u8 read + bytes written
  layout_us                cgen_nchw_to_nhwc(src_is_u8 = 1) on a resident u8 batch, same output view, same run (it neither gathers nor crops)
  step_ms / step_from_ms / host_ms
                           graph-replayed TrainStep.step on a resident u8 batch, TrainStep.step_from on index vectors, and the host path:
                           pinned u8 batch -> H2D copy -> step (h2d_ms: the copies alone)

The three step paths run on ONE model, interleaved in blocks (A B C A B C ...), each block timed by device events around its replays;
the figures are medians over the blocks, with the min..max spread next to them.  Needs a GPU: there is nothing to time without one."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import bench
from causal_gen_amd import _lib
from causal_gen_amd.data import DeviceDataset
from causal_gen_amd.train import TrainStep

NATIVE = {"morphomnist": 28, "cmnist": 28, "ukbb192": 192, "mimic192": 192, "mimic224": 224}


def timed(fn, reps):
    """ms per call of `fn`, device events around `reps` calls."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def med(v):
    return dict(median=round(statistics.median(v), 5), min=round(min(v), 5), max=round(max(v), 5))


def run(name, dtype, B, n_data, blocks, steps, kreps):
    lib = _lib.require_gpu()
    m, hp = bench.build_model(name, dtype)
    m = m.cuda().train()
    torch.manual_seed(7)
    ts = TrainStep(m, hp, ema=True, use_graph=True)
    eng = m.engine()
    g = torch.Generator().manual_seed(3)
    c, h0, R = hp.input_channels, NATIVE[name], hp.input_res
    x_all = torch.randint(0, 256, (n_data, c, h0, h0), generator=g, dtype=torch.uint8)
    pa_all = bench.synth_batch(name, hp, n_data, "cpu", 5)[1]
    pa_all = pa_all[:, :, 0, 0].contiguous() if pa_all.dim() == 4 else pa_all
    ds = DeviceDataset.from_args(hp, x_all, pa_all)
    r_h, r_w, px, py, p = ds.geometry(True)
    idx = [torch.randint(0, n_data, (B,), generator=g).cuda() for _ in range(8)]
    st = torch.cuda.current_stream().cuda_stream

    # ---- the kernel alone, next to the layout kernel on the same output view
    es = eng.es
    tdt = torch.float32 if es == 4 else (torch.bfloat16 if lib.h16_is_bf16 else torch.float16)
    out = torch.zeros((B, R, R, 8), dtype=tdt, device="cuda")
    view = _lib.View(out.data_ptr(), R * R * 8, R * 8, 8, c, 8)
    pa_out = torch.zeros((B, ds.ctx), device="cuda")
    a = ds.args_for(eng.dt, B, idx[0].data_ptr(), view, eng.rng_ptr(), True, None, None, pa_out.data_ptr())
    xb = torch.randint(0, 256, (B, c, R, R), generator=g, dtype=torch.uint8).cuda()
    k_aug = lambda: lib.batch_augment(C.byref(a), st)
    k_lay = lambda: lib.nchw_to_nhwc(1, eng.dt, B, c, R, R, xb.data_ptr(), view, 127.5, 1 / 127.5, st)
    for f in (k_aug, k_lay):
        timed(f, 20)
    t_aug, t_lay = [], []
    for _ in range(blocks):
        t_aug.append(1e3 * timed(k_aug, kreps))
        t_lay.append(1e3 * timed(k_lay, kreps))
    nbytes = B * c * R * R + B * R * R * 8 * es + B * ds.ctx * 8
    res = dict(config=name, dtype=dtype, batch=B, n_data=n_data, geometry=dict(h0=h0, r=R, pad_x=px, pad_y=py, hflip=p),
               kernel_us=med(t_aug), layout_us=med(t_lay), kernel_gbs=round(nbytes / (statistics.median(t_aug) * 1e-6) / 1e9, 1),
               kernel_bytes=nbytes)

    # ---- the three step paths, interleaved
    x_res = [x_all[i.cpu()][:, :, :R, :R] for i in idx]
    if h0 != R:  # the resident / host batches of step() are already at the model's resolution (the host pipeline padded them)
        x_res = [torch.nn.functional.pad(x, ((R - h0) // 2,) * 4) for x in x_res]
    x_pin = [x.contiguous().pin_memory() for x in x_res]
    pa_pin = [pa_all[i.cpu()].contiguous().pin_memory() for i in idx]
    x_dev, pa_dev = [x.cuda() for x in x_pin], [p_.cuda() for p_ in pa_pin]
    k = [0]

    def step_resident():
        k[0] += 1
        ts.step(x_dev[k[0] % 8], pa_dev[k[0] % 8])

    def step_from():
        k[0] += 1
        ts.step_from(ds, idx[k[0] % 8])

    def h2d():
        k[0] += 1
        return x_pin[k[0] % 8].to("cuda", non_blocking=True), pa_pin[k[0] % 8].to("cuda", non_blocking=True)

    def step_host():
        ts.step(*h2d())

    paths = (("step_ms", step_resident), ("step_from_ms", step_from), ("host_ms", step_host), ("h2d_ms", h2d))
    for _, f in paths:  # warm-up: eager step, capture (one graph per conditioning-dropout outcome), first replays
        torch.manual_seed(11)
        timed(f, 12)
    t = {nme: [] for nme, _ in paths}
    for _ in range(blocks):
        for nme, f in paths:
            torch.manual_seed(11)  # (cond_prior presets: every block sees the same sequence of host-side dropout outcomes)
            t[nme].append(timed(f, steps))
    res.update({nme: med(v) for nme, v in t.items()})
    s, sf, host, cp = (statistics.median(t[nme]) for nme, _ in paths)
    res["step_from_minus_step_us"] = round(1e3 * (sf - s), 2)
    res["host_minus_step_from_ms"] = round(host - sf, 4)
    res["n_skipped"] = ts.stats()["n_skipped"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="morphomnist,cmnist,ukbb192")
    ap.add_argument("--dtype", default="f16", choices=["f32", "f16"])
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30, help="replays per timed block")
    ap.add_argument("--kernel-reps", type=int, default=200)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_input.py needs a GPU: nothing here can be timed without one")
    for name in a.configs.split(","):
        small = NATIVE[name] <= 32
        line = json.dumps(run(name, a.dtype, 256 if small else 32, 8192 if small else 512, a.blocks, a.steps, a.kernel_reps))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
