"""The likelihood head alone at the flagship shape (32 x 192 x 192, 32 channels, f16): the fused launches cgen_dgauss_head_fwd / _bwd
against the launches they stand for, each timed by itself with HIP events -- 3 warm-up + 20 timed calls, the median.

usage: python tools/bench_like_head.py [--n 32] [--res 192] [--ci 32] [--which fused|separate|both]
Run each measurement as its own step with a time limit, e.g.
    timeout 120 python tools/bench_like_head.py --which separate && timeout 120 python tools/bench_like_head.py --which fused
Prints one line per launch: microseconds, the bytes the launch has to move, and that over the time against 6.3 TB/s."""
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


def image(w16, rows_of):
    """cgen_weight_prep's image of a [1, ci] 1x1 weight: mode 0 (rows = output channels) or mode 1 (rows = input channels)."""
    co, ci = w16.shape
    r, k = (co, ci) if rows_of == "co" else (ci, co)
    img = torch.zeros(ceil(r, 16), ceil(ceil(k, 8), 32) + 32, dtype=torch.float16)
    img[:r, :k] = w16 if rows_of == "co" else w16.t()
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
    print("%-34s %8.1f us   %7.1f MB   %5.2f TB/s (%4.1f %% of 6.3)" % (label, m, nbytes / 1e6, nbytes / m / 1e6, 100 * nbytes / (m * 1e-6) / PEAK))
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--res", type=int, default=192)
    ap.add_argument("--ci", type=int, default=32)
    ap.add_argument("--which", default="both", choices=["fused", "separate", "both"])
    a = ap.parse_args()
    lib = L.require_gpu()
    n, R, ci = a.n, a.res, a.ci
    P = n * R * R
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)
    h = torch.randn(P, ci, generator=g).half().cuda()
    gh = torch.zeros(P, ci, dtype=torch.float16, device="cuda")
    params = torch.zeros(P, 8, dtype=torch.float16, device="cuda")
    gparams = torch.zeros(P, 8, dtype=torch.float16, device="cuda")
    x = torch.zeros(P, 8, dtype=torch.float16)
    x[:, 0] = ((torch.randint(0, 256, (P,), generator=g).float() - 127.5) / 127.5).half()
    x = x.cuda()
    w_loc, w_ls = (torch.randn(1, ci, generator=g) * 0.05).half(), (torch.randn(1, ci, generator=g) * 0.05).half()
    b_loc, b_ls = torch.tensor([0.1]).cuda(), torch.tensor([-1.0]).cuda()
    f_loc, f_ls, d_loc, d_ls = image(w_loc, "co"), image(w_ls, "co"), image(w_loc, "ci"), image(w_ls, "ci")
    nchunk = lib.like_chunks(R, R)
    part = torch.zeros(n * nchunk, device="cuda")
    coef = torch.full((n,), 2.0 ** 14 / P, device="cuda")
    view = lambda t, c0, c1: L.View(t.data_ptr() + 2 * c0, R * R * t.shape[1], R * t.shape[1], t.shape[1], c1 - c0, 0)
    vh, vgh, vp, vx = view(h, 0, ci), view(gh, 0, ci), view(params, 0, 2), view(x, 0, 1)

    w = L.WgradArgs()
    w.dtype, w.n, w.h, w.w, w.ks, w.nseg, w.act = L.F16, n, R, R, 1, 1, L.ACT_NONE
    w.seg[0], w.gout = vh, view(gparams, 0, 1)
    kind = C.c_int32(-1)
    nsplit = lib.conv2d_wgrad_plan(C.byref(w), C.byref(kind))
    pw = [torch.zeros(nsplit * (ci + 1), device="cuda") for _ in range(2)]

    t = L.DgaussHeadArgs()
    t.dtype, t.n, t.h, t.w, t.hin, t.params, t.x = L.F16, n, R, R, vh, vp, vx
    t.img_loc, t.img_ls, t.bias_loc, t.bias_ls = f_loc.data_ptr(), f_ls.data_ptr(), b_loc.data_ptr(), b_ls.data_ptr()
    t.nll_part, t.coef_dev, t.coef_stride, t.nsplit, t.g_h, t.g_params = part.data_ptr(), coef.data_ptr(), 1, nsplit, vgh, L.NULL_VIEW
    t.partial_w_loc, t.partial_b_loc = pw[0].data_ptr(), pw[0].data_ptr() + 4 * nsplit * ci
    t.partial_w_ls, t.partial_b_ls = pw[1].data_ptr(), pw[1].data_ptr() + 4 * nsplit * ci
    if not lib.dgauss_head_supported(C.byref(t)):
        sys.exit("cgen_dgauss_head_supported: this shape is not served")

    def conv(seg, img, bias, out, res1):
        c = L.ConvArgs()
        c.dtype, c.n, c.h, c.w, c.ks, c.nseg, c.act, c.dact = L.F16, n, R, R, 1, 1, L.ACT_NONE, L.ACT_NONE
        c.seg[0], c.weight, c.bias, c.out, c.aux, c.res1, c.res2 = seg, img, bias, out, L.NULL_VIEW, res1, L.NULL_VIEW
        return lambda: lib.conv2d(C.byref(c), st)

    def wgrad(k):
        q = L.WgradArgs()
        q.dtype, q.n, q.h, q.w, q.ks, q.nseg, q.act, q.nsplit = L.F16, n, R, R, 1, 1, L.ACT_NONE, nsplit
        q.seg[0], q.gout = vh, view(gparams, k, k + 1)
        q.partial_w, q.partial_b = pw[k].data_ptr(), pw[k].data_ptr() + 4 * nsplit * ci
        return lambda: lib.conv2d_wgrad(C.byref(q), st)

    hb, pb, xb = 2 * P * ci, 4 * P, 2 * P
    lib.dgauss_head_fwd(C.byref(t), st)  # (the backward launches read real parameters)
    total = {}
    if a.which in ("separate", "both"):
        s = 0.0
        s += timed(conv(vh, f_loc.data_ptr(), b_loc.data_ptr(), view(params, 0, 1), L.NULL_VIEW), "conv x_loc (fwd)", hb + pb // 2)
        s += timed(conv(vh, f_ls.data_ptr(), b_ls.data_ptr(), view(params, 1, 2), L.NULL_VIEW), "conv x_logscale (fwd)", hb + pb // 2)
        s += timed(lambda: lib.dgauss_nll_fwd(L.F16, n, R, R, 1, vp, vx, part.data_ptr(), st), "dgauss_nll_fwd", pb + xb)
        total["separate forward"] = s
        s = 0.0
        s += timed(lambda: lib.dgauss_nll_bwd(L.F16, n, R, R, 1, vp, vx, coef.data_ptr(), 1, view(gparams, 0, 2), st), "dgauss_nll_bwd", 2 * pb + xb)
        s += timed(conv(view(gparams, 1, 2), d_ls.data_ptr(), None, vgh, L.NULL_VIEW), "dgrad x_logscale", hb + pb // 2)
        s += timed(conv(view(gparams, 0, 1), d_loc.data_ptr(), None, vgh, vgh), "dgrad x_loc (accumulating)", 2 * hb + pb // 2)
        s += timed(wgrad(1), "wgrad x_logscale", hb + pb // 2)
        s += timed(wgrad(0), "wgrad x_loc", hb + pb // 2)
        total["separate backward"] = s
    if a.which in ("fused", "both"):
        total["fused forward"] = timed(lambda: lib.dgauss_head_fwd(C.byref(t), st), "cgen_dgauss_head_fwd", hb + pb + xb)
        total["fused backward"] = timed(lambda: lib.dgauss_head_bwd(C.byref(t), st), "cgen_dgauss_head_bwd", 2 * hb + pb + xb)
    for k, v in total.items():
        print("%-20s %8.1f us" % (k, v))


if __name__ == "__main__":
    main()
