"""cgen_conv2d, forward and data gradient, called through the C ABI (cgen_weight_prep mode 0 / 1, then cgen_conv2d) on every case of
tests/conv_cases.py, against the f64 references and the tolerance of tests/conv_ref.py (its docstring derives every term; the
accumulation term is measured on the CPU from a sequential f32 chain, tests/test_conv_cases.py keeps the record).

Per case: cgen_conv2d_last_kernel() names the arm the dispatch mirror predicts; every output element meets the bound (no exclusions);
a second call gives the bits of the first; a data gradient that accumulates is also run in place (out and res1 one view), as the engine
runs it.  The weight image is compared bit for bit with one built on the host, once per (direction, ks, segment widths).

Layout: every view lies in a parent that is NaN wherever the view is not -- other samples, rows, columns and channels; only the
channels [c, cpad) of a view that declares cpad hold zeros, as include/cgen_hip.h promises.  Anything a kernel lets in from outside an
input view makes an output NaN; anything it writes outside the output view (beyond the zeros an output's cpad asks for, which must be
there) changes a parent that is compared bit for bit."""
import ctypes

import pytest
import torch

import conv_cases as T
import conv_ref as R
from gpu_views import U32, Arena, _bits, _ulp, assert_bounded, cv

pytestmark = pytest.mark.gpu
_IMAGES_CHECKED = set()


@pytest.fixture(scope="module")
def lib():
    from causal_gen_amd import _lib

    return _lib.require_gpu()


def _ceil(v, m):
    return -(-v // m) * m


def host_image(case, I):
    """The weight image cgen_weight_prep builds for the case: [rows_pad][krow], zero padded, in the storage format."""
    ks, taps = case.ks, case.ks * case.ks
    w = I.w  # OIHW f32
    if case.dir == "fwd":
        c8 = [_ceil(c, 8) for c in case.segs]
        ctot8, rows = sum(c8), case.co
        krow = _ceil(taps * ctot8, 32) + 32
        img = torch.zeros((_ceil(rows, 16), krow), dtype=torch.float32)
        body = img[:, :taps * ctot8].view(-1, taps, ctot8)
        wt = w.reshape(case.co, sum(case.segs), taps).permute(0, 2, 1)  # [co][tap][ci]
        k0 = s0 = 0
        for c, cp in zip(case.segs, c8):
            body[:rows, :, k0:k0 + c] = wt[:, :, s0:s0 + c]
            k0, s0 = k0 + cp, s0 + c
    else:
        co8, rows = _ceil(case.co, 8), case.out_c
        krow = _ceil(taps * co8, 32) + 32
        img = torch.zeros((_ceil(rows, 16), krow), dtype=torch.float32)
        body = img[:, :taps * co8].view(-1, taps, co8)
        wk = w[:, case.seg_off:case.seg_off + rows].reshape(case.co, rows, taps).flip(2)  # taps flipped
        body[:rows, :, :case.co] = wk.permute(1, 2, 0)  # [ci][tap][co]
    return img.to(I.tdt), krow


def device_image(lib, case, I):
    """cgen_weight_prep on the OIHW parameter; the image is followed by NaN."""
    from causal_gen_amd import _lib

    want, krow = host_image(case, I)
    rows_pad = want.shape[0]
    numel = rows_pad * krow
    src = I.w.contiguous().cuda()
    buf = torch.full((numel + 256,), float("nan"), dtype=I.tdt, device="cuda")
    d = _lib.WprepDesc()
    d.src, d.dst = src.data_ptr(), buf.data_ptr()
    d.co, d.ci_total, d.ks = case.co, sum(case.segs), case.ks
    if case.dir == "fwd":
        d.mode, d.nseg, d.seg_off = 0, len(case.segs), 0
        for k, c in enumerate(case.segs):
            d.seg_c[k] = c
    else:
        d.mode, d.nseg, d.seg_off = 1, 1, case.seg_off
        d.seg_c[0] = case.out_c
    d.dtype, d.rows_pad, d.k_pad, d.numel = (_lib.F16 if case.dt == "h16" else _lib.F32), rows_pad, krow, numel
    nch = -(-numel // 1024)
    tab = torch.frombuffer(bytearray(bytes(d)), dtype=torch.uint8).cuda()
    csite = torch.zeros(nch, dtype=torch.int32, device="cuda")
    cidx = torch.arange(nch, dtype=torch.int32, device="cuda")
    lib.weight_prep(tab.data_ptr(), csite.data_ptr(), cidx.data_ptr(), nch, None)
    torch.cuda.synchronize()
    key = (case.dir, case.dt, case.ks, case.segs, case.co, case.k)
    if key not in _IMAGES_CHECKED:
        _IMAGES_CHECKED.add(key)
        got = buf[:numel].view(rows_pad, krow).cpu()
        assert torch.equal(_bits(got), _bits(want)), "the weight image differs from the host-built one"
        assert bool(torch.isnan(buf[numel:]).all())
    return buf, src


class Run:
    """The parents, views and arguments of one case."""

    def __init__(self, lib, case, I, inplace=False):
        from causal_gen_amd import _lib

        self.lib, self.case, self.I = lib, case, I
        A = self.A = Arena(lib, case, None)
        A.tdt = I.tdt  # ("f32s" stores f32)
        n, h, w = case.n, case.h, case.w
        a = self.args = _lib.ConvArgs()
        a.dtype = {"f32": _lib.F32, "h16": _lib.F16, "f32s": _lib.F32S}[case.dt]
        a.n, a.h, a.w, a.ks, a.nseg = n, h, w, case.ks, len(case.in_segs)
        a.act, a.dact = (case.act, 0) if case.dir == "fwd" else (0, case.act)
        self.keep = []

        def put(role, values, out=False, planes=1):
            pshape, off, cpad = T.parent_shape(case, role)
            vs = A.place(pshape, off, (n, h, w, case.channels(role)), values, out=out, zero_to=0 if out else cpad, planes=planes)
            self.keep.append(vs)
            view = cv(vs[0], cpad)
            m = T.view(case, role)  # the mirror's picture of this view is the real one
            assert (view.p % 256, view.sn, view.sh, view.sw, view.c, view.cpad) == (m["p"], m["sn"], m["sh"], m["sw"], m["c"], m["cpad"])
            if planes == 2:
                assert vs[1].data_ptr() - vs[0].data_ptr() == T.rem_offset(case, role)
            return vs, view

        for s, x in enumerate(I.segs):
            _, a.seg[s] = put(f"s{s}", [x])
        self.img, self.src = device_image(lib, case, I)
        a.weight = self.img.data_ptr()
        self.bias = None
        if I.bias is not None:  # (followed by NaN, like the views: a group load past Co shows)
            self.bias = torch.full((case.out_c + 64,), float("nan"), device="cuda")
            self.bias[:case.out_c] = I.bias.cuda()
            assert self.bias.data_ptr() % 16 == 0
        a.bias = self.bias.data_ptr() if self.bias is not None else None
        if I.aux is not None:
            _, a.aux = put("aux", [I.aux])
        if I.res2 is not None:
            _, a.res2 = put("res2", [I.res2])
        oplanes = 2 if case.out_rem else 1
        if inplace:  # out and res1 are one view (and one remainder plane)
            assert case.layout("out") == case.layout("res1") and (not case.res1_rem or case.out_rem)
            self.out, a.out = put("out", [I.res1, I.res1_rem][:oplanes], out=True, planes=oplanes)
            a.res1 = a.out
            a.res1_rem = T.rem_offset(case, "out") if case.res1_rem else 0
        else:
            self.out, a.out = put("out", None, out=True, planes=oplanes)
            if I.res1 is not None:
                _, a.res1 = put("res1", [I.res1, I.res1_rem], planes=2 if case.res1_rem else 1)
                a.res1_rem = T.rem_offset(case, "res1") if case.res1_rem else 0
        a.out_rem = T.rem_offset(case, "out") if case.out_rem else 0
        self.cpad = T.parent_shape(case, "out")[2]

    def call(self):
        self.lib.conv2d(ctypes.byref(self.args), None)
        torch.cuda.synchronize()
        return self.lib.conv2d_last_kernel().decode()

    def check(self, ref):
        """The bound on `out` (and on out + its remainder plane), the zero padding, and everything around the views.  Returns the worst
        err / tol."""
        case, tdt = self.case, self.I.tdt
        off, oc = T.parent_shape(case, "out")[1], case.out_c
        pads = []
        for parent, v, before in self.A.outs:  # out, then its remainder plane: [c, cpad) of `out` holds zeros; of the plane, zeros or nothing
            pad = parent[:case.n, :case.h, :case.w, off + oc:off + self.cpad]
            was = before[:case.n, :case.h, :case.w, off + oc:off + self.cpad]
            if pads and torch.equal(_bits(pad), _bits(was)):
                pads.append(0)
                continue
            assert bool((pad == 0).all()), "channels [c, cpad) of the output are not zeros"
            pads.append(self.cpad)
        self.A.check_untouched(cpad=pads)
        got = self.out[0].cpu()
        assert bool(torch.isfinite(got).all()), f"{int((~torch.isfinite(got)).sum())} outputs are not finite: something from outside a view came in"
        tol = ref.k * U32 * ref.A_tol + _ulp(ref.ref, tdt)
        worst = float(((got.double() - ref.ref).abs() / tol.clamp_min(1e-300)).max())
        print(f"conv_f64 {T.family(case)} {case.id()} worst err/tol {worst:.3f} (k {ref.k:g})")
        assert_bounded(got, ref.ref, ref.A_tol, ref.k, tdt)
        if case.out_rem:
            rem = self.out[1].cpu()
            assert bool(torch.isfinite(rem).all())
            assert bool((rem.double().abs() <= 0.5 * _ulp(got.double(), tdt) * (1 + 2.0 ** -9)).all()), "the plane holds more than half an ulp of out"
            # out + out_rem: the bound with the output ulp replaced by one 16-bit ulp at the size of the plane value
            err = (got.double() + rem.double() - ref.ref).abs()
            tol2 = ref.k * U32 * ref.A_tol + _ulp(rem.double(), tdt)
            bad = ~(err <= tol2)
            assert not bad.any(), (f"out + out_rem: {int(bad.sum())} of {bad.numel()} outside the k={ref.k} bound; worst err/tol "
                                   f"{float((err / tol2.clamp_min(1e-300)).max()):.3g}")
        return worst

    def bits(self):
        return [_bits(v).clone() for v in self.out]


_REFS = {}


def _reference(case, bf16):
    if case.id() not in _REFS:
        _REFS.clear()  # (one case at a time: the big ones hold a few hundred MB in f64)
        I = R.make_inputs(case, bf16)
        _REFS[case.id()] = (I, R.reference(case, I))
    return _REFS[case.id()]


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id())
def test_conv_against_f64(lib, case, monkeypatch):
    I, ref = _reference(case, lib.h16_is_bf16)  # (on the CPU, before anything runs on the GPU)
    if case.dir == "fwd" and case.act == T.GELU and case.dt == "h16":
        assert ref.flag_share <= R.FLAG_SHARE_MAX
    for name in T.ALL_FORCE_ENV:
        monkeypatch.delenv(name, raising=False)
    for name in T.FORCE_ENV[case.force]:
        monkeypatch.setenv(name, "1")
    want = T.arm(case)
    run = Run(lib, case, I)
    assert run.call() == want, f"cgen_conv2d_last_kernel(): the mirror expects {want}"
    run.check(ref)
    first = run.bits()
    assert run.call() == want
    for a, b in zip(first, run.bits()):
        assert torch.equal(a, b), "a second call gives other bits"
    if case.dir == "dgrad" and case.res1:
        inp = Run(lib, case, I, inplace=True)
        assert inp.call() == want
        inp.check(ref)
        for a, b in zip(first, inp.bits()):
            assert torch.equal(a, b), "the in-place accumulate gives other bits"
