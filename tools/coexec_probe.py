#!/usr/bin/env python3
"""Is a fused light-Block launch (csrc/block.hip: blk3s / blk3 / blk3r) bit-stable beside a packed weight-gradient batch?

One Block is run once through the engine (forward and backward) with the two `cgen_block3` calls recorded; each recorded launch is
then replayed on fixed inputs, alone (the reference: every byte of the arena the pass used) and `reps` times while one packed
weight-gradient batch (`cgen_conv2d_wgrad_batch_run`, the flush's 304-workgroup grid cap, copies of a 64 -> 16 3x3 problem at 96^2,
B = 32) runs on a second stream.  Every byte must be the same as alone.  This is the kernel-level form of LABNOTES 12 (4-9 of 2500
train steps with a non-finite encoder gradient when the flush ran beside the backward chain); the packed-f32 erratum of LABNOTES 3.4
was found with a probe of the same kind.

usage: python tools/coexec_probe.py [--cases blk3s12,blk3_24,...] [--reps 100] [--batch 32] [--copies 8] [--dirs fwd,bwd] [--quiet-wgrad]
a case is name[:batch[:reps[:dirs joined by +]]], e.g. blk3s12:256:4000:bwd (the form in which the unfixed small-image kernel shows
its stale reads within seconds: 6 of 4000 launches differed); prints one JSON line per case and exits 1 when a launch differed;
CGEN_CONV_TRACE=1 in the environment shows on stderr which instance each launch took.
CGEN_LIB=<another build> probes that build (a -DB3_DRAIN_WAITS one, for instance)."""
import argparse
import ctypes as C
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from causal_gen_amd import _lib  # noqa: E402

# name -> (H, W, channels in, bottleneck, channels out): one case per instance of csrc/block.hip at the smallest ukbb192-like shape
# that selects it; the batch (32) makes tiles per workgroup match the workload
CASES = {
    "blk3s6": (6, 6, 160, 40, 160),      # small-image instance, one workgroup per image
    "blk3s12": (12, 12, 160, 40, 160),   # ... four strips of three rows per image
    "blk3_24": (24, 24, 128, 32, 128),   # tile instance, eight-row tiles
    "blk3_48": (48, 48, 96, 24, 96),     # tile instance, twelve-row tiles
    "blk3r96": (96, 96, 64, 16, 64),     # row-streaming instance
}
WG_CAP = 304  # the grid cap of the engine's background flush (Engine.wgrad_bg_wgs)


def record_block(N, H, W, ci, b, co, seed=0):
    """One light Block with a residual through the engine; returns (engine, [forward Block3Args], [data-gradient Block3Args], keep)."""
    from causal_gen_amd.engine import ConvSite, Engine

    g = torch.Generator().manual_seed(1000 * seed + H * 7 + co)
    c1 = torch.nn.Conv2d(ci, b, 3, padding=1)
    c2 = torch.nn.Conv2d(b, co, 3, padding=1)
    with torch.no_grad():
        c1.weight.copy_(torch.randn(c1.weight.shape, generator=g) / math.sqrt(ci * 9 / 2))
        c2.weight.copy_(torch.randn(c2.weight.shape, generator=g) / math.sqrt(b * 9 / 2))
        c1.bias.copy_(torch.randn(b, generator=g) * 0.2)
        c2.bias.copy_(torch.randn(co, generator=g) * 0.2)
    x = torch.randn(N, ci, H, W, generator=g).half().float()
    res = torch.randn(N, co, H, W, generator=g).half().float()
    gout = torch.randn(N, co, H, W, generator=g).half().float()
    eng = Engine("cuda", "f16")
    eng.blk3_on, eng.blk3_minres = 2, 8
    eng.blk3_res, eng.blk3_res3 = [], []
    eng.wgrad_flush_frac = []  # (the Block's own weight gradients: one in-line batch at the end of the pass)
    holder = torch.nn.ModuleList([c1, c2]).cuda()
    s1 = ConvSite("c1", holder[0], [ci], [True], 0)
    s2 = ConvSite("c2", holder[1], [b], [True], 1)
    s1.blk3, s2.blk3 = ("a", s2), ("b", s1)
    eng.bind(holder, [s1, s2])
    eng.begin()
    eng.prepare_weights(force=True)
    rec = []
    lib = eng.lib
    orig = lib.block3

    def recording_block3(a, stream):
        rec.append(_lib.Block3Args.from_buffer_copy(bytes(a._obj)))
        return orig(a, stream)

    lib.block3 = recording_block3
    try:
        eng.recording = True
        xt = eng.from_nchw(x.cuda(), rg=True)
        rt = eng.from_nchw(res.cuda(), rg=False)
        y = eng.block2(s1, s2, [xt], 1, res1=rt)
        gy = eng.seed_grad(y)
        eng.lib.axpby(eng.dt, N, H, W, eng.from_nchw(gout.cuda()).cv(), gy.cv(), 1.0, 1.0, 1 << 30, 0, eng.stream)
        eng.recording = False
        eng.backward()
        torch.cuda.synchronize()
    finally:
        lib.block3 = orig
    fwd = [a for a in rec if a.pre_act]
    bwd = [a for a in rec if not a.pre_act]
    assert len(fwd) == 1 and len(bwd) == 1, "the Block did not take cgen_block3 in both directions: %d forward, %d data-gradient launches" % (len(fwd), len(bwd))
    return eng, fwd[0], bwd[0], (holder, s1, s2, xt, rt, y, gy)


def aggressor(lib, copies):
    """`2 * copies` weight-gradient problems 64 -> 16, 3x3, 96^2, B = 32 as one packed batch; returns a launcher and what it keeps alive."""
    N, H, W, ci, co = 32, 96, 96, 64, 16
    g = torch.Generator(device="cuda").manual_seed(5)
    xt = torch.randn(N, H, W, ci, device="cuda", generator=g).half()
    gt = torch.randn(N, H, W, co, device="cuda", generator=g).half()
    a0 = _lib.WgradArgs()
    a0.dtype, a0.n, a0.h, a0.w, a0.ks, a0.nseg, a0.act = 1, N, H, W, 3, 1, 1
    a0.seg[0] = _lib.View(xt.data_ptr(), xt.stride(0), xt.stride(1), xt.stride(2), ci, 0)
    a0.gout = _lib.View(gt.data_ptr(), gt.stride(0), gt.stride(1), gt.stride(2), co, 0)
    nsplit = lib.conv2d_wgrad_plan(C.byref(a0), None)
    nw = co * 9 * ci
    parts, args = [], []
    for _ in range(2 * copies):
        part = torch.empty(nsplit * (nw + co), dtype=torch.float32, device="cuda")
        a = _lib.WgradArgs.from_buffer_copy(bytes(a0))
        a.nsplit, a.partial_w, a.partial_b = nsplit, part.data_ptr(), part.data_ptr() + 4 * nsplit * nw
        parts.append(part)
        args.append(a)
    n = len(args)
    arr = (_lib.WgradArgs * n)(*args)
    nbytes, nl = C.c_int64(0), C.c_int32(0)
    elig = (C.c_int32 * n)()
    lib.conv2d_wgrad_batch_plan(arr, n, None, 0, C.byref(nbytes), None, 0, C.byref(nl), elig)
    host = (C.c_char * max(nbytes.value, 1))()
    launches = (_lib.WgradBatchLaunch * max(nl.value, 1))()
    lib.conv2d_wgrad_batch_plan(arr, n, host, nbytes.value, C.byref(nbytes), launches, nl.value, C.byref(nl), elig)
    assert all(elig[i] for i in range(n)) and nl.value >= 1, "the packed kernel does not serve the aggressor's problems"
    blob = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).cuda()

    def launch(stream):
        lib.conv2d_wgrad_batch_run(blob.data_ptr(), launches, nl.value, WG_CAP, stream.cuda_stream)

    return launch, (xt, gt, parts, blob, launches, arr)


def probe(name, N, reps, copies, dirs, with_wgrad=True):
    H, W, ci, b, co = CASES[name]
    eng, fwd, bwd, keep = record_block(N, H, W, ci, b, co)
    lib = eng.lib
    main = torch.cuda.current_stream()  # (the engine launches on it)
    side = torch.cuda.Stream()
    launch_wg, keep_wg = aggressor(lib, copies)
    assert eng.arena.ci == 0, "the pass fits one arena chunk"
    used = eng.arena.chunks[0][:eng.arena.off]
    out = {"case": name, "n": N, "h": H, "w": W, "channels": [ci, b, co], "reps": reps, "wgrad_beside": bool(with_wgrad),
           "supported": [int(lib.block3_supported(C.byref(fwd))), int(lib.block3_supported(C.byref(bwd)))]}
    # how long the two last: the batch has to outlast the victim
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    launch_wg(main)
    torch.cuda.synchronize()
    e[0].record(); launch_wg(main); e[1].record()
    torch.cuda.synchronize()
    out["wgrad_batch_us"] = round(e[0].elapsed_time(e[1]) * 1e3, 1)
    for d, a in (("fwd", fwd), ("bwd", bwd)):
        if d not in dirs:
            continue
        for _ in range(2):
            lib.block3(C.byref(a), eng.stream)
        torch.cuda.synchronize()
        e[2].record(); lib.block3(C.byref(a), eng.stream); e[3].record()
        torch.cuda.synchronize()
        out[d + "_alone_us"] = round(e[2].elapsed_time(e[3]) * 1e3, 1)
        ref = used.clone()
        bad = torch.zeros((), dtype=torch.int64, device="cuda")
        for r in range(reps):
            if with_wgrad:
                launch_wg(side)
            lib.block3(C.byref(a), eng.stream)
            bad += (used != ref).any()
            if r % 32 == 31:  # (bounds the queue of batches on the second stream)
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        out[d + "_reps_differing"] = int(bad)
        assert out[d + "_alone_us"] < out["wgrad_batch_us"] or not with_wgrad, ("the batch does not outlast the victim: more --copies", out)
        del ref
    del keep, keep_wg
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--copies", type=int, default=8)
    ap.add_argument("--dirs", default="fwd,bwd")
    ap.add_argument("--quiet-wgrad", action="store_true", help="no batch beside the victim (control: must always give 0)")
    o = ap.parse_args()
    _lib.require_gpu()
    worst = 0
    for spec in o.cases.split(","):
        f = spec.split(":")
        batch = int(f[1]) if len(f) > 1 and f[1] else o.batch
        reps = int(f[2]) if len(f) > 2 and f[2] else o.reps
        dirs = f[3].split("+") if len(f) > 3 and f[3] else o.dirs.split(",")
        r = probe(f[0], batch, reps, o.copies, dirs, with_wgrad=not o.quiet_wgrad)
        r["spec"] = spec
        worst = max(worst, r.get("fwd_reps_differing", 0), r.get("bwd_reps_differing", 0))
        print(json.dumps(r), flush=True)
    return 1 if worst else 0


if __name__ == "__main__":
    sys.exit(main())
