"""The discretised-Gaussian likelihood head as one launch each way (csrc/likelihood.hip, cgen_dgauss_head_fwd / _bwd).

Kernel level, through the C ABI, on views laid out as the engine lays them out (h inside a wider parent whose rows are longer than
the image is wide; the 2-channel parameter tensor with a pixel stride of 8 channels):
  forward   against cgen_conv2d x 2 + cgen_dgauss_nll_fwd: every byte of the parameter buffer (padding channels included) and of the
            NLL partials (guard band included);
  backward  against cgen_dgauss_nll_bwd + the two data-gradient cgen_conv2d calls in tape order (x_logscale stores, x_loc accumulates)
            + cgen_conv2d_wgrad x 2 + cgen_wgrad_reduce_tiles: every byte of grad(h)'s parent, of both sites' weight and bias partials
            and of the reduced f32 gradients (reduced with `accumulate` onto a non-zero gradient, unscaled by a power-of-two loss scale).
That the comparison ran the kernels whose arithmetic was copied is what cgen_dgauss_head_supported() == 1 says: it asks cgen_conv2d's
own decision (conv_tile_kernel in one K-step, not the small-image kernel) and cgen_conv2d_wgrad_plan (the generic kernel).

f64 case: the fused launches' outputs against an f64 restatement on the binary16 inputs, with the bounds tests/test_gpu_ops.py uses for
the f16 1x1 conv (rtol = atol = 3e-2; weight gradients rtol 5e-2, atol 5e-2 sqrt(P) / 4) and for the DGauss kernels (NLL per sample
rtol 2e-5, atol 1e-6; parameter gradients rtol 2e-3, atol 1e-5 max|g| + 1e-7).

Model level: a small f16 HVAE whose 64 x 64 top resolution is served, CGEN_LIKE_HEAD=1 against =0 on the same weights and noise."""
import ctypes as C
import zlib
from types import SimpleNamespace

import pytest
import torch

EUNSUPPORTED = -3
LIKE_PIX = 1024
GUARD = 64
# (n, h, w): 2 x 56 x 56 = 6 272 pixels (above the small-image kernel's 6 000; 3 136 pixels per sample leave the last 1024-pixel chunk
# ragged; 25 weight-gradient splits of 256 pixels, one across the sample boundary, the last one half full); 3 x 48 x 64: non-square
SHAPES = [(2, 56, 56), (3, 48, 64)]
CHANNELS = [32, 16]
_bits16 = lambda x: x.view(torch.int16)
_bits32 = lambda x: x.view(torch.int32)


def _lib():
    from causal_gen_amd import _lib

    return _lib


def _ceil(a, m):
    return (a + m - 1) // m * m


def _fwd_image(w16):
    """cgen_weight_prep mode 0 for a 1x1 conv of one segment: row = output channel (padded to 16), ceil32(ceil8(ci)) + 32 columns."""
    co, ci = w16.shape
    img = torch.zeros(_ceil(co, 16), _ceil(_ceil(ci, 8), 32) + 32, dtype=torch.float16)
    img[:co, :ci] = w16
    return img


def _dgrad_image(w16):
    """cgen_weight_prep mode 1 for a 1x1 conv: img[r][k] = W[k][r]."""
    co, ci = w16.shape
    img = torch.zeros(_ceil(ci, 16), _ceil(_ceil(co, 8), 32) + 32, dtype=torch.float16)
    img[:ci, :co] = w16.t()
    return img


def wgrad_plan(P):
    """The generic weight-gradient kernel's split plan for one output channel and up to 32 input channels (csrc/like_head.h)."""
    nsplit = max(1, min(2048, -(-P // 256)))
    pps = _ceil(-(-P // nsplit), 64)
    return -(-P // pps), pps


class Case:
    def __init__(self, shape, ci, mild=False):
        n, h, w = shape
        self.n, self.h, self.w, self.ci, self.P = n, h, w, ci, n * h * w
        g = torch.Generator().manual_seed(zlib.crc32(repr((shape, ci, mild)).encode()))
        rn = lambda *s: torch.randn(*s, generator=g)
        P = self.P
        self.hx = (rn(P, ci) * (1.0 if mild else 3.0)).half()
        if mild:  # (f64 case: scales near 1 and means near the pixels, where the f32 CDF difference keeps its digits)
            self.w_loc, self.w_ls = (rn(1, ci) * 0.01).half(), (rn(1, ci) * 0.01).half()
            self.b_loc, self.b_ls = torch.tensor([0.1]), torch.tensor([0.2])
        else:  # log-scale pre-activations from far below the -9 clamp to large ones
            self.w_loc, self.w_ls = (rn(1, ci) * 0.05).half(), (rn(1, ci) * 0.5).half()
            self.b_loc, self.b_ls = torch.tensor([-0.07]), torch.tensor([-3.0])
        x = (torch.randint(0, 256, (P, 1), generator=g).float() - 127.5) / 127.5
        x[::7] = -1.0  # edge bins
        x[3::11] = 1.0
        self.x = x.half()
        self.S = 2.0 ** 14  # power-of-two loss scale
        self.coef = torch.tensor([0.75, 1.375][:n] + [1.0] * max(0, n - 2)) * self.S / (P * 8.0)
        self.nchunk = _ceil(h * w, LIKE_PIX) // LIKE_PIX
        self.nsplit, self.pps = wgrad_plan(P)

    # ---- device staging
    def stage(self):
        n, h, w, ci = self.n, self.h, self.w, self.ci
        e = SimpleNamespace()
        self.wp, self.cpar, self.coff = w + 3, ci + 16, 8  # h: rows 3 pixels longer than the image, 8 channels in front, 8 behind

        def wide(t, fill):
            parent = torch.full((n, h, self.wp, self.cpar), fill, dtype=torch.float16)
            parent[:, :, :w, self.coff:self.coff + ci] = t.view(n, h, w, ci)
            return parent.cuda()

        e.h = wide(self.hx, 5.0)
        e.gh = wide(torch.full((self.P, ci), 77.0, dtype=torch.float16), 77.0)
        e.params = torch.full((n, h, w, 8), 77.0, dtype=torch.float16).cuda()
        e.gparams = torch.full((n, h, w, 8), 77.0, dtype=torch.float16).cuda()
        xx = torch.full((n, h, w, 8), 9.0, dtype=torch.float16)
        xx[..., 0] = self.x.view(n, h, w)
        e.x = xx.cuda()
        e.part = torch.full((n * self.nchunk + GUARD,), -5.0, device="cuda")
        e.img_loc, e.img_ls = _fwd_image(self.w_loc).cuda(), _fwd_image(self.w_ls).cuda()
        e.dg_loc, e.dg_ls = _dgrad_image(self.w_loc).cuda(), _dgrad_image(self.w_ls).cuda()
        e.b_loc, e.b_ls = self.b_loc.cuda(), self.b_ls.cuda()
        e.coef = self.coef.cuda()
        npart = self.nsplit * (ci + 1)
        e.pw_loc = torch.full((npart + GUARD,), -5.0, device="cuda")
        e.pw_ls = torch.full((npart + GUARD,), -5.0, device="cuda")
        g = torch.Generator().manual_seed(9)
        e.grad = (torch.randn(2 * (ci + 1), generator=g) * 0.1).cuda()  # [w_loc | b_loc | w_ls | b_ls], non-zero: the reduce accumulates
        return e

    def v_h(self, t):
        L = _lib()
        return L.View(t.data_ptr() + 2 * self.coff, self.h * self.wp * self.cpar, self.wp * self.cpar, self.cpar, self.ci, 0)

    def v_p(self, t, c0=0, c1=2):
        L = _lib()
        return L.View(t.data_ptr() + 2 * c0, self.h * self.w * 8, self.w * 8, 8, c1 - c0, 0)

    def args(self, e, gparams=True):
        L = _lib()
        t = L.DgaussHeadArgs()
        t.dtype, t.n, t.h, t.w = L.F16, self.n, self.h, self.w
        t.hin, t.params, t.x = self.v_h(e.h), self.v_p(e.params), self.v_p(e.x, 0, 1)
        t.img_loc, t.img_ls, t.bias_loc, t.bias_ls = e.img_loc.data_ptr(), e.img_ls.data_ptr(), e.b_loc.data_ptr(), e.b_ls.data_ptr()
        t.nll_part = e.part.data_ptr()
        t.coef_dev, t.coef_stride, t.nsplit = e.coef.data_ptr(), 1, self.nsplit
        t.g_h = self.v_h(e.gh)
        t.g_params = self.v_p(e.gparams) if gparams else L.NULL_VIEW
        nw = self.nsplit * self.ci
        t.partial_w_loc, t.partial_b_loc = e.pw_loc.data_ptr(), e.pw_loc.data_ptr() + 4 * nw
        t.partial_w_ls, t.partial_b_ls = e.pw_ls.data_ptr(), e.pw_ls.data_ptr() + 4 * nw
        return t

    # ---- today's launches
    def _conv(self, lib, seg, img, bias, out, res1, st):
        L = _lib()
        a = L.ConvArgs()
        a.dtype, a.n, a.h, a.w, a.ks, a.nseg, a.act, a.dact = L.F16, self.n, self.h, self.w, 1, 1, L.ACT_NONE, L.ACT_NONE
        a.seg[0], a.weight, a.bias, a.out = seg, img, bias, out
        a.aux, a.res1, a.res2 = L.NULL_VIEW, res1, L.NULL_VIEW
        lib.conv2d(C.byref(a), st)

    def launches_fwd(self, e, lib, st):
        L = _lib()
        self._conv(lib, self.v_h(e.h), e.img_loc.data_ptr(), e.b_loc.data_ptr(), self.v_p(e.params, 0, 1), L.NULL_VIEW, st)
        self._conv(lib, self.v_h(e.h), e.img_ls.data_ptr(), e.b_ls.data_ptr(), self.v_p(e.params, 1, 2), L.NULL_VIEW, st)
        lib.dgauss_nll_fwd(L.F16, self.n, self.h, self.w, 1, self.v_p(e.params), self.v_p(e.x, 0, 1), e.part.data_ptr(), st)

    def launches_bwd(self, e, lib, st):
        L = _lib()
        lib.dgauss_nll_bwd(L.F16, self.n, self.h, self.w, 1, self.v_p(e.params), self.v_p(e.x, 0, 1), e.coef.data_ptr(), 1,
                           self.v_p(e.gparams), st)
        nw = self.nsplit * self.ci
        for k, dg, pw in ((1, e.dg_ls, e.pw_ls), (0, e.dg_loc, e.pw_loc)):  # tape order: x_logscale first
            w = L.WgradArgs()
            w.dtype, w.n, w.h, w.w, w.ks, w.nseg, w.act = L.F16, self.n, self.h, self.w, 1, 1, L.ACT_NONE
            w.seg[0], w.gout = self.v_h(e.h), self.v_p(e.gparams, k, k + 1)
            kind = C.c_int32(-1)
            assert lib.conv2d_wgrad_plan(C.byref(w), C.byref(kind)) == self.nsplit and kind.value == 0
            w.nsplit, w.partial_w, w.partial_b = self.nsplit, pw.data_ptr(), pw.data_ptr() + 4 * nw
            lib.conv2d_wgrad(C.byref(w), st)
            self._conv(lib, self.v_p(e.gparams, k, k + 1), dg.data_ptr(), None, self.v_h(e.gh),
                       self.v_h(e.gh) if k == 0 else L.NULL_VIEW, st)

    def reduce(self, e, lib, st):
        """Both sites' partials -> e.grad (+=), as the engine's reduce round does it."""
        from causal_gen_amd.wgrad_sched import plan_wred_items

        L = _lib()
        ci, nw = self.ci, self.nsplit * self.ci
        descs = []
        for j, pw in enumerate((e.pw_loc, e.pw_ls)):
            d = L.WredDesc()
            d.partial_w, d.partial_b = pw.data_ptr(), pw.data_ptr() + 4 * nw
            d.grad_w, d.grad_b = e.grad.data_ptr() + 4 * j * (ci + 1), e.grad.data_ptr() + 4 * (j * (ci + 1) + ci)
            d.co, d.ci_total, d.ks, d.nsplit, d.layout, d.accumulate, d.unscale, d.numel = 1, ci, 1, self.nsplit, 0, 1, 1.0 / self.S, ci + 1
            descs.append(d)
        items = plan_wred_items(descs)
        dev = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).cuda()
        lib.wgrad_reduce_tiles(dev.data_ptr(), len(items), st)
        torch.cuda.synchronize()


_REF = {}


def _reference(shape, ci):
    """Today's launches, run once per (shape, channels) and shared: (case, the staged buffers after the nine launches and the reduce)."""
    key = (shape, ci)
    if key not in _REF:
        lib = _lib().require_gpu()
        case = Case(shape, ci)
        e = case.stage()
        st = torch.cuda.current_stream().cuda_stream
        case.launches_fwd(e, lib, st)
        case.launches_bwd(e, lib, st)
        case.reduce(e, lib, st)
        _REF[key] = (case, e)
    return _REF[key]


@pytest.mark.gpu
@pytest.mark.parametrize("ci", CHANNELS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_equals_the_three_launches_bit_for_bit(shape, ci):
    lib = _lib().require_gpu()
    case, ref = _reference(shape, ci)
    e = case.stage()
    t = case.args(e)
    assert lib.dgauss_head_supported(C.byref(t)) == 1  # (conv_tile_kernel in one K-step serves the convs; the generic wgrad plan)
    lib.dgauss_head_fwd(C.byref(t), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    pr = ref.params.float()
    assert (pr[..., 1] < -9.0).any() and (pr[..., 1] > 5.0).any()  # the clamp and large log-scales are both in play
    bad = _bits16(e.params) != _bits16(ref.params)
    assert not bad.any(), (int(bad.sum()), bad.numel())
    assert (e.params[..., 2:] == 77.0).all()  # the padding channels keep their fill
    assert torch.equal(_bits32(e.part), _bits32(ref.part)), (e.part - ref.part).abs().max().item()
    assert (e.part[case.n * case.nchunk:] == -5.0).all() and torch.isfinite(e.part).all()
    assert (e.gh == 77.0).all() and (e.gparams == 77.0).all() and (e.pw_loc == -5.0).all()  # a forward call writes nothing else
    h0 = case.stage().h
    assert torch.equal(_bits16(e.h), _bits16(h0))


@pytest.mark.gpu
@pytest.mark.parametrize("ci", CHANNELS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_equals_the_six_launches_and_the_reduce_bit_for_bit(shape, ci):
    lib = _lib().require_gpu()
    case, ref = _reference(shape, ci)
    if shape == (2, 56, 56):  # the plan this shape is here for
        assert (case.nsplit, case.pps) == (25, 256)
        assert (case.h * case.w) % case.pps != 0 and case.P % case.pps != 0  # a split across the sample boundary, a ragged last one
    st = torch.cuda.current_stream().cuda_stream
    for with_gparams in (True, False):
        e = case.stage()
        e.params.copy_(ref.params)
        t = case.args(e, gparams=with_gparams)
        lib.dgauss_head_bwd(C.byref(t), st)
        case.reduce(e, lib, st)
        if with_gparams:
            assert torch.equal(_bits16(e.gparams), _bits16(ref.gparams))
        else:
            assert (e.gparams == 77.0).all()
        bad = _bits16(e.gh) != _bits16(ref.gh)
        assert not bad.any(), (int(bad.sum()), bad.numel())
        inner = e.gh[:, :, :case.w, case.coff:case.coff + ci]
        assert torch.isfinite(inner.float()).all() and not (inner == 77.0).all()
        for nm in ("pw_loc", "pw_ls"):
            got, want = getattr(e, nm), getattr(ref, nm)
            assert torch.equal(_bits32(got), _bits32(want)), (nm, (got - want).abs().max().item())
            assert (got[case.nsplit * (ci + 1):] == -5.0).all() and torch.isfinite(got).all()
        assert torch.equal(_bits32(e.grad), _bits32(ref.grad)), (e.grad - ref.grad).abs().max().item()
        assert (e.part == -5.0).all()  # a backward call leaves the forward's outputs alone
        assert torch.equal(_bits16(e.params), _bits16(ref.params))


def _declined():
    L = _lib()
    out = []

    def make(shape=(2, 56, 56), ci=32, mutate=None):
        case = Case(shape, ci)
        case.wp, case.cpar, case.coff = case.w + 3, ci + 16, 8
        h = torch.zeros(1, dtype=torch.float16)  # only addresses and layouts are looked at
        base = (h.data_ptr() + 255) // 256 * 256
        e = SimpleNamespace(**{k: SimpleNamespace(data_ptr=lambda base=base: base) for k in
                               ("h", "gh", "params", "gparams", "x", "part", "img_loc", "img_ls", "b_loc", "b_ls", "coef", "pw_loc", "pw_ls")})
        t = case.args(e)
        if mutate:
            mutate(t)
        return t

    out.append(("served", make(), 1))
    out.append(("served, 16 channels", make(ci=16), 1))
    out.append(("f32", make(mutate=lambda t: setattr(t, "dtype", L.F32)), 0))

    def rgb(t):
        t.x = L.View(t.x.p, t.x.sn, t.x.sh, t.x.sw, 3, 0)
        t.params = L.View(t.params.p, t.params.sn * 2, t.params.sh * 2, 16, 9, 0)

    out.append(("C = 3", make(mutate=rgb), 0))
    out.append(("3 136 pixels: the small-image kernel serves the convs", make(shape=(1, 56, 56)), 0))
    out.append(("a 4-pixel-wide image", make(shape=(40, 50, 4)), 0))
    out.append(("64 input channels", make(mutate=lambda t: setattr(t, "hin", L.View(t.hin.p, t.hin.sn, t.hin.sh, t.hin.sw, 64, 0))), 0))
    out.append(("h off by 8 bytes", make(mutate=lambda t: setattr(t, "hin", L.View(t.hin.p + 8, t.hin.sn, t.hin.sh, t.hin.sw, t.hin.c, 0))), 0))
    out.append(("no bias", make(mutate=lambda t: setattr(t, "bias_ls", None)), 0))
    return out


def test_supported_answers_without_a_gpu_and_declined_calls_return_the_error_code():
    lib = _lib().load()
    for label, t, want in _declined():
        assert lib.dgauss_head_supported(C.byref(t)) == want, label
        if not want:
            for fn in (lib._raw_cgen_dgauss_head_fwd, lib._raw_cgen_dgauss_head_bwd):
                assert fn(C.byref(t), None) == EUNSUPPORTED, label
                assert b"cgen_dgauss_head" in lib.cdll.cgen_last_error()


def test_backward_declines_a_split_count_that_is_not_the_plan():
    lib = _lib().load()
    t = _declined()[0][1]
    t.nsplit += 1
    assert lib._raw_cgen_dgauss_head_bwd(C.byref(t), None) == EUNSUPPORTED


# ----------------------------------------------------------------------------- f64
K0, K1 = 0.79788456080286535588, 0.044715


def _nll64(loc, ls, x):
    ls = ls.clamp(min=-9.0)
    inv, d = torch.exp(-ls), x - loc
    cdf = lambda u: 0.5 * (1.0 + torch.tanh(K0 * (u + K1 * u ** 3)))
    cp, cm = cdf(inv * (d + 1.0 / 255.0)), cdf(inv * (d - 1.0 / 255.0))
    lp = torch.where(x < -0.999, cp.clamp(min=1e-12).log(), torch.where(x > 0.999, (1.0 - cm).clamp(min=1e-12).log(), (cp - cm).clamp(min=1e-12).log()))
    return -lp


@pytest.mark.gpu
def test_fused_launches_against_an_f64_restatement():
    lib = _lib().require_gpu()
    case = Case((2, 56, 56), 32, mild=True)
    e = case.stage()
    st = torch.cuda.current_stream().cuda_stream
    t = case.args(e)
    assert lib.dgauss_head_supported(C.byref(t)) == 1
    lib.dgauss_head_fwd(C.byref(t), st)
    lib.dgauss_head_bwd(C.byref(t), st)
    e.grad.zero_()
    case.reduce(e, lib, st)
    n, h, w, ci, P = case.n, case.h, case.w, case.ci, case.P
    H, X = case.hx.double(), case.x.double()[:, 0]
    wl, ws = case.w_loc.double()[0], case.w_ls.double()[0]
    # heads: the f16 1x1 conv's bound
    got = e.params.cpu().view(P, 8)[:, :2].double()
    want = torch.stack([H @ wl + case.b_loc.double(), H @ ws + case.b_ls.double()], 1)
    torch.testing.assert_close(got, want, rtol=3e-2, atol=3e-2)
    # NLL and its gradient on the parameters the kernel stored: the DGauss kernels' bounds
    p = got.clone().requires_grad_(True)
    nll = _nll64(p[:, 0], p[:, 1], X)
    part = e.part[:n * case.nchunk].cpu().double().view(n, case.nchunk).sum(1) / (h * w)
    torch.testing.assert_close(part, nll.detach().view(n, h * w).mean(1), rtol=2e-5, atol=1e-6)
    coef = case.coef.double().repeat_interleave(h * w)
    (g_ref,) = torch.autograd.grad((nll * coef).sum(), p)
    gp = e.gparams.cpu().view(P, 8)[:, :2].double()
    torch.testing.assert_close(gp, g_ref, rtol=2e-3, atol=1e-5 * g_ref.abs().max().item() + 1e-7)
    # grad(h) and the weight gradients from the gradients the kernel used (gp): the f16 conv's bounds
    gh = e.gh.cpu().view(n, h, case.wp, case.cpar)[:, :, :w, case.coff:case.coff + ci].reshape(P, ci).double()
    torch.testing.assert_close(gh, gp[:, :1] * wl[None] + gp[:, 1:] * ws[None], rtol=3e-2, atol=3e-2)
    gw = e.grad.cpu().double().view(2, ci + 1) * case.S
    wtol = dict(rtol=5e-2, atol=5e-2 * (P ** 0.5) / 4)
    for j in range(2):
        torch.testing.assert_close(gw[j, :ci], gp[:, j] @ H, **wtol)
        torch.testing.assert_close(gw[j, ci], gp[:, j].sum(), **wtol)


# ----------------------------------------------------------------------------- model level
def _small_hp(**over):
    from causal_gen_amd.hps import setup_hparams

    return setup_hparams("ukbb192", input_res=64, enc_arch="64b1d2,32b1d4,8b1d8,1b1", dec_arch="1b1,8b1,32b1,64b1",
                         widths=[32, 32, 64, 64], z_max_res=32, z_dim=8, bs=2, **over)


def _small_model(hp, freeze_ls=False):
    from causal_gen_amd import vae

    torch.manual_seed(7)
    m = vae.HVAE(hp)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for p in m.parameters():  # (the reference zero-initialises some heads: every conv gets weight)
            p.add_(torch.randn(p.shape, generator=g) * 0.05)
    if freeze_ls:
        m.likelihood.x_logscale.weight.requires_grad = False
    m.compute_dtype = "f16"
    return m.cuda().train()


def _batch(hp, B=2):
    g = torch.Generator().manual_seed(1)
    R = hp.input_res
    x = (torch.randint(0, 256, (B, 1, R, R), generator=g).float() - 127.5) / 127.5
    pa = torch.randn(B, hp.context_dim, generator=g)
    return x.cuda(), pa.cuda()[..., None, None].expand(-1, -1, R, R)


def _seed(eng):
    eng.rng_ptr()
    eng.rng.copy_(torch.tensor([11, 0], dtype=torch.int64, device=eng.rng.device))


def _one_pass(monkeypatch, knob, freeze_ls=False):
    monkeypatch.setenv("CGEN_LIKE_HEAD", knob)
    hp = _small_hp()
    m = _small_model(hp, freeze_ls)
    x, pa = _batch(hp)
    eng = m.engine()
    _seed(eng)
    l0 = eng.launches
    out = m(x, pa, beta=2.0)
    out["elbo"].backward()
    torch.cuda.synchronize()
    launches, heads = eng.launches - l0, eng.like_heads
    vals = {k: out[k].detach().cpu().clone() for k in ("elbo", "nll", "kl")}
    grads = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters() if p.grad is not None}
    return vals, grads, launches, heads


def _same(a, b):
    (v1, g1), (v0, g0) = a, b
    for k in v0:
        assert torch.equal(v1[k], v0[k]), (k, v1[k], v0[k])
    assert set(g1) == set(g0)
    for n in g0:
        assert torch.equal(g1[n], g0[n]), (n, float((g1[n].double() - g0[n].double()).abs().max()))


@pytest.mark.gpu
def test_model_two_launches_against_nine(monkeypatch):
    """ELBO, NLL, KL and every parameter gradient keep their bits.  Forward + backward launches: the two convs and the NLL become one
    launch (-2); the zero fill of the parameter gradient's padding channels, the NLL's backward, two data gradients and two weight
    gradients become one (-5).  Seven launches fewer in all."""
    _lib().require_gpu()
    v1, g1, n1, h1 = _one_pass(monkeypatch, "1")
    v0, g0, n0, h0 = _one_pass(monkeypatch, "0")
    print("forward + backward launches: separate %d, fused %d" % (n0, n1))
    assert (h0, h1) == (0, 2)
    assert n0 - n1 >= 5 and n0 - n1 == 7, (n0, n1)
    _same((v1, g1), (v0, g0))
    assert "likelihood.x_loc.weight" in g1 and "likelihood.x_logscale.bias" in g1


@pytest.mark.gpu
def test_model_with_a_frozen_logscale_weight_is_declined_and_unchanged(monkeypatch):
    _lib().require_gpu()
    v1, g1, n1, h1 = _one_pass(monkeypatch, "1", freeze_ls=True)
    v0, g0, n0, h0 = _one_pass(monkeypatch, "0", freeze_ls=True)
    assert (h0, h1, n0) == (0, 0, n1)
    _same((v1, g1), (v0, g0))


@pytest.mark.gpu
def test_train_step_graph_replay_equals_eager_on_the_fused_path(monkeypatch):
    from causal_gen_amd.train import TrainStep

    _lib().require_gpu()
    outs = []
    for knob, use_graph in (("1", False), ("1", True), ("0", True)):
        monkeypatch.setenv("CGEN_LIKE_HEAD", knob)
        hp = _small_hp(lr=2e-3, lr_warmup_steps=2)
        m = _small_model(hp)
        x, pa = _batch(hp)
        torch.manual_seed(123)
        ts = TrainStep(m, SimpleNamespace(**vars(hp)), ema=True, use_graph=use_graph)
        for _ in range(3):
            o = ts.step(x, pa)
        torch.cuda.synchronize()
        assert m.engine().like_heads == (2 if knob == "1" else 0)
        outs.append(([float(v) for v in o.cpu()], {k: v.clone() for k, v in m.state_dict().items()}))
    for o1, s1 in outs[1:]:
        assert outs[0][0] == o1, (outs[0][0], o1)
        for k in s1:
            assert torch.equal(outs[0][1][k], s1[k]), k
