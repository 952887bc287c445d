"""Element-wise NHWC kernels (csrc/elementwise.hip) called through the C ABI on views over torch tensors, against an f64 torch
reference, over the case table of tests/elementwise_cases.py: both dtypes, the vector / scalar / flat arms, channel-slice views,
accumulation, odd sizes and grid-stride wrap.

Tolerances.  Data movement (broadcast, plain transposes, im2col, nearest upsampling) and the relu / leaky_relu / clamp_min / add forward
and backward must match bit for bit (up to the sign of zero): the kernel does at most one f32 operation per element (two for an
accumulated gradient) and rounds once to the storage format, and the reference does the same operations.
Sums, axpby, the scaled transpose and GELU are held to  k * 2^-24 * (the same computation on absolute values)  -- the classic bound of a k-term f32
sum -- plus, in 16 bits, one unit in the last place of the output format; the 16-bit reference runs on the 16-bit-rounded
inputs.  Every output lives in a parent tensor filled with NaN: what the call must not write is compared bit for bit after it."""
import math
import types
import zlib

import pytest
import torch
import torch.nn.functional as F

import elementwise_cases as E
from gpu_views import U32, Arena, _bits, _cdt, _tdt, _ulp, assert_bounded, assert_exact, cv, f32  # noqa: F401

pytestmark = pytest.mark.gpu

OPS = {"relu": 1, "gelu": 2, "leaky_relu": 3, "clamp_min": 4, "add": 5}


@pytest.fixture(scope="module")
def lib():
    from causal_gen_amd import _lib

    return _lib.require_gpu()


def nchw(v):
    return v.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def _autograd(fn, x64, g64):
    x = x64.clone().requires_grad_(True)
    fn(x).backward(g64)
    return x.grad


def _edges(x, u, param, with_nan):
    """Edge values in place: exact zeros (relu / leaky_relu kinks), x == min (clamp_min), NaN, |x| up to 10 (GELU)."""
    idx = torch.arange(x.numel(), device="cuda")
    vals = x.reshape(-1).clone()
    vals[idx % 7 == 0] = 0.0
    if u == "clamp_min":
        vals[idx % 11 == 3] = param
    if u == "gelu":
        vals = vals.clamp(-10, 10)
        vals[idx % 13 == 5] = 10.0
        vals[idx % 13 == 6] = -10.0
    if with_nan:
        vals[idx % 17 == 9] = float("nan")
    x.copy_(vals.view(x.shape))


def _run(lib, case):
    st = torch.cuda.current_stream().cuda_stream
    A = Arena(lib, case, E.parent_shape)
    tdt, dt, op, acc = A.tdt, _cdt(case.dt), case.op, case.acc
    V = E.views(case)
    written = None

    if op == "avgpool_fwd":
        d, = case.p
        x, y = A.view(V["in"]), A.view(V["out"], out=True, init=False)
        lib.avgpool_fwd(dt, case.n, case.h, case.w, d, cv(x), cv(y), st)
        x64 = nchw(x).double()
        check = lambda: assert_bounded(y, nhwc(F.avg_pool2d(x64, d)), nhwc(F.avg_pool2d(x64.abs(), d)), d * d + 3, tdt)  # noqa: E731
    elif op in ("avgpool_bwd", "adaptive_avgpool_bwd", "upsample_bwd"):
        go, gi = A.view(V["gout"]), A.view(V["out"], out=True, init=bool(acc))
        gi0 = gi.double().clone()
        n, h, w, c = V["out"]
        _, ho, wo, _ = V["gout"]
        if op == "avgpool_bwd":
            d, = case.p
            lib.avgpool_bwd(dt, n, ho, wo, d, cv(go), cv(gi), acc, st)
            fn, k = (lambda t: F.avg_pool2d(t, d)), 3
        elif op == "adaptive_avgpool_bwd":
            lib.adaptive_avgpool_bwd(dt, n, h, w, ho, wo, cv(go), cv(gi), acc, st)
            fn, k = (lambda t: F.adaptive_avg_pool2d(t, (ho, wo))), 2 * 4 + 3  # <= 4 windows hold a pixel; 2 roundings each
        else:
            lib.upsample_bwd(dt, n, h, w, ho, wo, cv(go), cv(gi), acc, st)
            fn, k = (lambda t: F.interpolate(t, scale_factor=(ho / h, wo / w), mode="nearest")), (ho // h + 2) * (wo // w + 2) + 2
        g64 = nchw(go).double()
        z = torch.zeros(n, c, h, w, dtype=torch.float64, device="cuda")

        def check():
            ref = nhwc(_autograd(fn, z, g64)) + (gi0 if acc else 0)
            ab = nhwc(_autograd(fn, z, g64.abs())) + (gi0.abs() if acc else 0)
            assert_bounded(gi, ref, ab, k, tdt)
    elif op == "adaptive_avgpool_fwd":
        hi, wi = case.p
        x, y = A.view(V["in"]), A.view(V["out"], out=True, init=False)
        lib.adaptive_avgpool_fwd(dt, case.n, hi, wi, case.h, case.w, cv(x), cv(y), st)
        x64 = nchw(x).double()
        k = (hi // case.h + 2) * (wi // case.w + 2) + 3
        check = lambda: assert_bounded(y, nhwc(F.adaptive_avg_pool2d(x64, (case.h, case.w))),  # noqa: E731
                                       nhwc(F.adaptive_avg_pool2d(x64.abs(), (case.h, case.w))), k, tdt)
    elif op == "upsample_fwd":
        hi, wi, with_bias = case.p
        x, y = A.view(V["in"]), A.view(V["out"], out=True, init=False)
        bias = A.rand((case.h, case.w, case.c)) if with_bias else None
        lib.upsample_fwd(dt, case.n, hi, wi, case.h, case.w, cv(x), bias.data_ptr() if with_bias else None, cv(y), st)
        up = nhwc(F.interpolate(nchw(x).double(), scale_factor=(case.h / hi, case.w / wi), mode="nearest"))
        ref = (up.float() + bias).to(tdt) if with_bias else up.to(tdt)  # (one f32 addition, rounded once)
        check = lambda: assert_exact(y, ref)  # noqa: E731
    elif op == "batch_broadcast":
        src = A.rand((case.h, case.w, case.c))
        y = A.view(V["out"], out=True, init=False)
        lib.batch_broadcast(dt, case.n, case.h, case.w, src.data_ptr(), cv(y), st)
        check = lambda: assert_exact(y, src.expand(case.n, -1, -1, -1).to(tdt))  # noqa: E731
    elif op == "axpby":
        from causal_gen_amd import _lib

        alpha, beta, c_from, fill = case.p
        if case.flat_axpy:
            from causal_gen_amd.engine import Engine

            count = case.c
            src = A.rand((count,))
            y = A.flat_out(count, bool(acc))
            y0 = y.double().clone()
            eng = types.SimpleNamespace(lib=lib, stream=st, launches=0)
            Engine.flat_axpy(eng, src.data_ptr(), y.data_ptr(), count, alpha=alpha, accumulate=bool(acc))
            assert eng.launches == len(E.flat_axpy_calls(count))
            x64, scale = src.double(), alpha
        else:
            x = None if fill else A.view(V["in"])
            y = A.view(V["out"], out=True, init=bool(acc))
            y0 = y.double().clone()
            lib.axpby(dt, case.n, case.h, case.w, _lib.NULL_VIEW if fill else cv(x), cv(y), alpha, beta, c_from, acc, st)
            ch = torch.arange(case.c, device="cuda")
            scale = alpha if fill else torch.where(ch >= c_from, alpha * beta, alpha).double()  # (a fill ignores beta)
            x64 = torch.ones_like(y0) if fill else x.double()

        def check():  # alpha * beta, the product and the sum: three f32 roundings
            t = x64 * scale
            assert_bounded(y, t + (y0 if acc else 0), t.abs() + (y0.abs() if acc else 0), 4, tdt)
    elif op == "batch_reduce":
        unscale, = case.p
        x = A.view(V["in"])
        out = A.flat_out(case.h * case.w * case.c, bool(acc))
        o0 = out.double().clone()
        lib.batch_reduce(dt, case.n, case.h, case.w, cv(x), out.data_ptr(), acc, unscale, st)
        x64 = x.double()

        def check():
            ref = x64.sum(0).reshape(-1) * unscale + (o0 if acc else 0)
            ab = x64.abs().sum(0).reshape(-1) * abs(unscale) + (o0.abs() if acc else 0)
            assert_bounded(out, ref, ab, case.n + 3, torch.float32)
    elif op == "nchw_to_nhwc":
        src_kind, sub, mul = case.p
        n, h, w, c = V["out"]
        if src_kind == "u8":
            src = torch.randint(0, 256, (n, c, h, w), generator=A.g, device="cuda", dtype=torch.uint8)
        else:
            src = A.rand((n, c, h, w), scale=3.0)
        y = A.view(V["out"], out=True, init=False)
        lib.nchw_to_nhwc(1 if src_kind == "u8" else 0, dt, n, c, h, w, src.data_ptr(), cv(y), sub, mul, st)
        if sub == 0.0 and mul == 1.0:  # a plain transpose: bit for bit
            check = lambda: assert_exact(y, nhwc(src.float()).to(tdt))  # noqa: E731
        else:  # (x - sub) * mul: two f32 roundings (the compiler may fuse the product with the 16-bit rounding)
            x64 = nhwc(src.double())
            check = lambda: assert_bounded(y, (x64 - f32(sub)) * f32(mul), (x64.abs() + abs(f32(sub))) * abs(f32(mul)), 3, tdt)  # noqa: E731
    elif op == "nhwc_to_nchw":
        n, h, w, c = V["in"]
        x = A.view(V["in"])
        dst = A.flat_out(n * c * h * w, False)
        lib.nhwc_to_nchw(dt, n, c, h, w, cv(x), dst.data_ptr(), st)
        check = lambda: assert_exact(dst.view(n, c, h, w), nchw(x).float())  # noqa: E731
    elif op == "im2col_strided":
        ks, stride, pad, cpad = case.p
        x = A.view(V["in"])
        n, ho, wo, cc = V["out"]
        y = A.view(V["out"], out=True, init=False)
        cphys = max(cc, cpad)
        written = y.as_strided((n, ho, wo, cphys), y.stride())  # (channels [c ks^2, cpad) are written as zeros)
        lib.im2col_strided(dt, case.n, case.h, case.w, ks, stride, pad, ho, wo, cv(x), cv(y, cpad), st)
        cols = F.unfold(nchw(x).double(), ks, padding=pad, stride=stride).view(n, cc, ho, wo)
        ref = torch.cat([nhwc(cols), torch.zeros(n, ho, wo, cphys - cc, dtype=torch.float64, device="cuda")], 3).to(tdt)
        check = lambda: assert_exact(written, ref)  # noqa: E731
    elif op == "col2im_strided":
        ks, stride, pad = case.p
        gcol = A.view(V["gcol"])
        gi = A.view(V["out"], out=True, init=bool(acc))
        gi0 = gi.double().clone()
        n, ho, wo, cc = V["gcol"]
        lib.col2im_strided(dt, case.n, case.h, case.w, ks, stride, pad, ho, wo, cv(gcol), cv(gi), acc, st)
        g64 = nchw(gcol).double().reshape(n, cc, ho * wo)
        fold = lambda t: nhwc(F.fold(t, (case.h, case.w), ks, padding=pad, stride=stride))  # noqa: E731
        k = ((ks + stride - 1) // stride) ** 2 + 2

        def check():
            assert_bounded(gi, fold(g64) + (gi0 if acc else 0), fold(g64.abs()) + (gi0.abs() if acc else 0), k, tdt)
    elif op in ("unary_fwd", "unary_bwd"):
        u, param = case.p
        x = A.view(V["out"], scale=4.0 if u == "gelu" else 1.0)
        _edges(x, u, param, with_nan=(op == "unary_fwd" and u in ("relu", "leaky_relu", "clamp_min")))
        x64, x32 = x.double(), x.float()
        p32 = torch.tensor(param, dtype=torch.float32, device="cuda")
        torch_op = {"relu": torch.relu, "gelu": F.gelu, "leaky_relu": lambda t: F.leaky_relu(t, param),
                    "clamp_min": lambda t: torch.clamp_min(t, param), "add": lambda t: t + param}[u]
        if op == "unary_fwd":
            y = A.view(V["out"], out=True, init=False)
            lib.unary_fwd(dt, OPS[u], param, case.n, case.h, case.w, case.c, cv(x), cv(y), st)
            if u == "gelu":
                ab = 0.5 * x64.abs() * (1 + torch.erf(x64 * 0.5 ** 0.5).abs())
                check = lambda: assert_bounded(y, F.gelu(x64), ab, 16, tdt)  # noqa: E731  (erff: a few ulp)
            else:  # the op in f32 with the f32 parameter, as the engine defines it
                ref32 = {"relu": torch.relu(x32), "leaky_relu": torch.where(x32 > 0, x32, x32 * p32),
                         "clamp_min": torch.clamp_min(x32, p32), "add": x32 + p32}[u]
                check = lambda: assert_exact(y, ref32.to(tdt))  # noqa: E731
        else:
            go = A.view(V["out"])
            gi = A.view(V["out"], out=True, init=bool(acc))
            gi0 = gi.float().clone()
            lib.unary_bwd(dt, OPS[u], param, case.n, case.h, case.w, case.c, cv(x), cv(go), cv(gi), acc, st)
            df64 = _autograd(torch_op, x64, torch.ones_like(x64))  # torch's gradient at the kinks: relu'(0) = 0, clamp passes at min
            if u == "gelu":
                pdf = torch.exp(-0.5 * x64 * x64) / math.sqrt(2 * math.pi)
                ab = go.double().abs() * (0.5 * (1 + torch.erf(x64 * 0.5 ** 0.5).abs()) + x64.abs() * pdf)
                check = lambda: assert_bounded(gi, go.double() * df64 + (gi0.double() if acc else 0),  # noqa: E731
                                               ab + (gi0.double().abs() if acc else 0), 32, tdt)  # (__expf: (1 + |arg|) 2^-23)
            else:
                ref = (go.float() * df64.float() + (gi0 if acc else 0)).to(tdt)  # (0, 1 or the f32 slope; one product, one sum)
                check = lambda: assert_exact(gi, ref)  # noqa: E731
    else:
        raise KeyError(op)

    torch.cuda.synchronize()
    check()
    A.check_untouched(written)


@pytest.mark.parametrize("case", E.CASES, ids=[c.id() for c in E.CASES])
def test_elementwise(lib, case):
    _run(lib, case)
