"""A deterministic decoder layer's latent tail alone at the flagship shape (32 x 192 x 192, C = 32, Z = 16, ctx = 4, f16): the fused
launches (cgen_latent_tail_fwd / _bwd without q_loc / q_ls) against the launches they stand for, each timed by itself with HIP events
-- 3 warm-up + 20 timed calls, the median.

usage: python tools/bench_det_tail.py [--n 32] [--res 192] [--c 32] [--z 16] [--which fused|separate|both]
Run each measurement as its own step with a time limit, e.g.
    timeout 120 python tools/bench_det_tail.py --which separate && timeout 120 python tools/bench_det_tail.py --which fused
Prints one line per launch: microseconds, the bytes the launch has to move (every tensor once; pout's 2Z + C channels count whole
where a launch reads or writes a slice of every pixel's 128-byte line), and that over the time against 6.3 TB/s."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from causal_gen_amd import _lib as L  # noqa: E402

PEAK = 6.3e12


def ceil(a, m):
    return (a + m - 1) // m * m


def fwd_image(w16, seg_c):
    co = w16.shape[0]
    img = torch.zeros(ceil(co, 16), ceil(sum(ceil(c, 8) for c in seg_c), 32) + 32, dtype=torch.float16)
    src = dst = 0
    for c in seg_c:
        img[:co, dst:dst + c] = w16[:, src:src + c]
        src, dst = src + c, dst + ceil(c, 8)
    return img.cuda()


def dgrad_image(w16, off, c):
    co = w16.shape[0]
    img = torch.zeros(ceil(c, 16), ceil(ceil(co, 8), 32) + 32, dtype=torch.float16)
    img[:c, :co] = w16[:, off:off + c].t()
    return img.cuda()


def timed(fn, label, nbytes):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    m = statistics.median(us)
    print("%-44s %8.1f us   %7.1f MB   %5.2f TB/s (%4.1f %% of 6.3)" % (label, m, nbytes / 1e6, nbytes / m / 1e6, 100 * nbytes / (m * 1e-6) / PEAK))
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--res", type=int, default=192)
    ap.add_argument("--c", type=int, default=32)
    ap.add_argument("--z", type=int, default=16)
    ap.add_argument("--ctx", type=int, default=4)
    ap.add_argument("--which", default="both", choices=["fused", "separate", "both"])
    a = ap.parse_args()
    lib = L.require_gpu()
    n, R, Cw, Z, ctx = a.n, a.res, a.c, a.z, a.ctx
    P = n * R * R
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g).half().cuda()
    pout, h, g_h, g_f = rn(P, 2 * Z + Cw), rn(P, Cw), rn(P, Cw), rn(P, Cw)
    h2, zf, gp = [torch.zeros(P, c, dtype=torch.float16, device="cuda") for c in (Cw, Cw, 2 * Z + Cw)]
    pa = torch.zeros(n, 8, dtype=torch.float16)
    pa[:, :ctx] = torch.randn(n, ctx, generator=g).half()
    pa = pa.cuda()
    w_p, w_f = (torch.randn(Cw, Z + ctx, generator=g) * 0.2).half(), (torch.randn(Cw, Z + Cw, generator=g) * 0.1).half()
    img_p, img_f = fwd_image(w_p, [Z, ctx]), fwd_image(w_f, [Z, Cw])
    img_pz, img_fz, img_fp = dgrad_image(w_p, 0, Z), dgrad_image(w_f, 0, Z), dgrad_image(w_f, Z, Cw)
    b_p, b_f = torch.zeros(Cw, device="cuda"), torch.zeros(Cw, device="cuda")
    view = lambda t, c0, c1: L.View(t.data_ptr() + 2 * c0, R * R * t.shape[1], R * t.shape[1], t.shape[1], c1 - c0, 0)
    v_pl, v_pf, v_pa = view(pout, 0, Z), view(pout, 2 * Z, 2 * Z + Cw), L.View(pa.data_ptr(), 8, 0, 0, ctx, 8)
    g_l, g_s, g_pf = view(gp, 0, Z), view(gp, Z, 2 * Z), view(gp, 2 * Z, 2 * Z + Cw)

    def fwd_args(feat):
        t = L.LatentTailFwdArgs()
        t.dtype, t.n, t.h, t.w, t.z_dim, t.c, t.ctx = L.F16, n, R, R, Z, Cw, ctx
        t.p_loc, t.p_feat, t.h_in, t.pa = v_pl, v_pf, view(h, 0, Cw), v_pa
        t.q_loc = t.q_ls = t.p_ls = t.eps = t.z = L.NULL_VIEW
        t.h_out, t.zf = view(h2, 0, Cw), (view(zf, 0, Cw) if feat else L.NULL_VIEW)
        t.img_p, t.img_f, t.bias_p, t.bias_f = img_p.data_ptr(), (img_f.data_ptr() if feat else None), b_p.data_ptr(), (b_f.data_ptr() if feat else None)
        if not lib.latent_tail_fwd_supported(C.byref(t)):
            sys.exit("cgen_latent_tail_fwd_supported: this shape is not served")
        return t

    def bwd_args(feat):
        t = L.LatentTailArgs()
        t.dtype, t.n, t.h, t.w, t.z_dim, t.c, t.parity = L.F16, n, R, R, Z, Cw, 1
        t.g_h, t.g_f = view(g_h, 0, Cw), (view(g_f, 0, Cw) if feat else L.NULL_VIEW)
        t.gz_in = t.q_loc = t.q_ls = t.p_loc = t.p_ls = t.z = t.out_q = L.NULL_VIEW
        t.out_p, t.img_pz = view(gp, 0, 2 * Z + Cw), img_pz.data_ptr()
        if feat:
            t.img_fz, t.img_fp = img_fz.data_ptr(), img_fp.data_ptr()
        if not lib.latent_tail_bwd_supported(C.byref(t)):
            sys.exit("cgen_latent_tail_bwd_supported: this shape is not served")
        return t

    def conv(segs, img, bias, out, res1, res2):
        c = L.ConvArgs()
        c.dtype, c.n, c.h, c.w, c.ks, c.nseg, c.act, c.dact = L.F16, n, R, R, 1, len(segs), L.ACT_NONE, L.ACT_NONE
        for k, s in enumerate(segs):
            c.seg[k] = s
        c.weight, c.bias, c.out, c.aux, c.res1, c.res2 = img.data_ptr(), bias, out, L.NULL_VIEW, res1, res2
        return lambda: lib.conv2d(C.byref(c), st)

    axpby = lambda src, dst, alpha, acc: (lambda: lib.axpby(L.F16, n, R, R, src, dst, alpha, 1.0, 1 << 30, acc, st))
    NV = L.NULL_VIEW
    cb, pb, zb = 2 * P * Cw, 2 * P * (2 * Z + Cw), 2 * P * Z  # a C-channel tensor, pout or its gradient, a Z-channel slice
    total = {}
    if a.which in ("separate", "both"):
        z_proj = timed(conv([v_pl, v_pa], img_p, b_p.data_ptr(), view(h2, 0, Cw), view(h, 0, Cw), v_pf), "conv z_proj (fwd; + h + p_feat)", pb + 2 * cb)
        total["separate forward, layer with z_feat_proj"] = z_proj + timed(conv([v_pl, v_pf], img_f, b_f.data_ptr(), view(zf, 0, Cw), NV, NV), "conv z_feat_proj (fwd)", pb + cb)
        total["separate forward, last layer"] = z_proj
        s = timed(conv([view(g_f, 0, Cw)], img_fz, None, g_l, NV, NV), "dgrad z_feat_proj -> grad(p_loc)", cb + zb)
        s += timed(conv([view(g_f, 0, Cw)], img_fp, None, g_pf, NV, NV), "dgrad z_feat_proj -> grad(p_feat)", 2 * cb)
        s += timed(axpby(view(g_h, 0, Cw), g_pf, 1.0, 1), "axpby grad(p_feat) += g_h (the rider)", 3 * cb)
        s += timed(conv([view(g_h, 0, Cw)], img_pz, None, g_l, g_l, NV), "dgrad z_proj -> grad(p_loc) (accumulating)", cb + 2 * zb)
        fill = timed(axpby(NV, g_s, 0.0, 0), "fill grad(p_ls) = 0", zb)
        total["separate backward, layer with z_feat_proj"] = s + fill
        s = timed(axpby(view(g_h, 0, Cw), g_pf, 1.0, 0), "axpby grad(p_feat) = g_h (the rider)", 2 * cb)
        s += timed(conv([view(g_h, 0, Cw)], img_pz, None, g_l, NV, NV), "dgrad z_proj -> grad(p_loc)", cb + zb)
        total["separate backward, last layer"] = s + fill
    if a.which in ("fused", "both"):
        for feat, name in ((True, "layer with z_feat_proj"), (False, "last layer")):
            tf, tb = fwd_args(feat), bwd_args(feat)
            total["fused forward, " + name] = timed(lambda: lib.latent_tail_fwd(C.byref(tf), st), "cgen_latent_tail_fwd (det), " + name, pb + (3 if feat else 2) * cb)
            total["fused backward, " + name] = timed(lambda: lib.latent_tail_bwd(C.byref(tb), st), "cgen_latent_tail_bwd (det), " + name, pb + (2 if feat else 1) * cb)
    for k, v in total.items():
        print("%-44s %8.1f us" % (k, v))


if __name__ == "__main__":
    main()
