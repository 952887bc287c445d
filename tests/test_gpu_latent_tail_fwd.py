"""The forward latent tail of a stochastic decoder layer as one launch (csrc/latent_tail.hip, cgen_latent_tail_fwd).

Kernel level, through the C ABI on views that are channel slices of wider parents, as the engine passes them: z, kl_part, h' and
zf must have the bits that cgen_reparam_kl_fwd + cgen_conv2d (z_proj: res1 = h, res2 = p_feat) + cgen_conv2d (z_feat_proj) leave
through the same ABI, every element checked, at shapes served by either conv kernel (conv_smallp up to 6 000 pixels, conv_px
above).  What the call must not write -- the neighbouring channels of the parents, h, the q / p buffers -- is compared bit for
bit after it.

f64 sanity, one case per serving kernel, against an f64 CPU reference built from the binary16 inputs and weights:
    z:        one binary16 rounding of q_loc + exp(q_ls + logt) eps (2^-10 |v|, plus the f32 evaluation 2^-22 A, plus 2^-24)
    h', zf:   |out - v| <= 2^-10 |v| + (K + 16) 2^-24 A + 2^-24 per element, K = the GEMM's terms, A = the f64 sum of |terms|, the GEMM
              taken over the z the kernel stored
    kl_part:  |out - v| <= (n + 32) 2^-24 A for the n <= 2048 terms of a chunk (an f32 sum of n terms, each a few roundings)
This catches an error the fused and the three launches would share.

Model level: the small f16 HVAE of tests/test_gpu_latent_tail.py, CGEN_LAT_TAIL_FWD=1 against =0 on the same weights and Philox state."""
import ctypes as C
import math
import zlib
from types import SimpleNamespace

import pytest
import torch

from latent_tail_cases import _batch, _ceil, _fwd_image, _lib, _same, _seed, _small_model

EUNSUPPORTED = -3
# (n, h, w, C, Z): conv_smallp serves the first five (<= 6 000 pixels; 20 * 24 * 16 elements leave a partial last KL chunk, 24 * 24
# has 4.5 chunks per sample), conv_px the last two (6 912 and 6 336 pixels; the second with the 7-K-step instance and partial chunks)
SHAPES = [(3, 6, 6, 192, 16), (2, 12, 12, 160, 16), (1, 20, 24, 32, 16), (2, 24, 24, 128, 16), (2, 12, 12, 96, 8),
          (3, 48, 48, 64, 16), (11, 24, 24, 160, 16)]
VARIANTS = {
    "philox-paconst-ctx4-cf_same": dict(eps=False, pa_const=True, ctx=4, zf="same"),
    "eps-pamat-ctx20-cf_narrow": dict(eps=True, pa_const=False, ctx=20, zf="narrow"),
    "philox-pamat-ctx4-nozf": dict(eps=False, pa_const=False, ctx=4, zf="none"),
    "eps-paconst-ctx20-cf_same": dict(eps=True, pa_const=True, ctx=20, zf="same"),
}
LAT_CHUNK = 2048


class Case:
    def __init__(self, shape, variant):
        B, H, W, Cw, Z = shape
        v = VARIANTS[variant]
        self.shape, self.variant = shape, variant
        self.B, self.H, self.W, self.C, self.Z, self.ctx = B, H, W, Cw, Z, v["ctx"]
        self.has_eps, self.pa_const = v["eps"], v["pa_const"]
        self.Cf = {"same": Cw, "narrow": max(32, (Cw // 2) // 32 * 32), "none": 0}[v["zf"]]
        g = torch.Generator().manual_seed(zlib.crc32(repr((shape, variant)).encode()))
        P = self.P = B * H * W
        rn = lambda *s: torch.randn(*s, generator=g)
        ru = lambda lo, hi, *s: torch.rand(*s, generator=g) * (hi - lo) + lo
        self.q_loc, self.p_loc = rn(P, Z).half(), rn(P, Z).half()
        self.q_ls, self.p_ls = ru(-2.0, 1.0, P, Z).half(), ru(-2.0, 1.0, P, Z).half()
        self.p_feat, self.h = rn(P, Cw).half(), (rn(P, Cw) * 3.0).half()
        self.eps = rn(P, Z).half()
        pa = rn(B, self.ctx)
        self.pa = (pa if self.pa_const else pa.repeat_interleave(H * W, 0) + 0.25 * rn(P, self.ctx)).half()
        self.w_p, self.b_p = (rn(Cw, Z + self.ctx) * 0.2).half(), rn(Cw) * 0.5
        self.w_f, self.b_f = (rn(max(self.Cf, 1), Z + Cw) * 0.1).half(), rn(max(self.Cf, 1)) * 0.5
        self.logt = math.log(0.9)
        self.stream_id = 1003
        self.chunks = _ceil(H * W * Z, LAT_CHUNK) // LAT_CHUNK
        self.kl_stride = self.chunks + 3

    def put(self, t, c_off=8, c_extra=16):
        P, c = t.shape
        parent = torch.randn(P, c + c_extra, generator=torch.Generator().manual_seed(5)).half()
        parent[:, c_off:c_off + c] = t
        return parent.cuda(), c_off, c

    def view(self, ent, c0=0, c1=None):
        L = _lib()
        parent, off, c = ent
        c1 = c if c1 is None else c1
        sw = parent.shape[1]
        return L.View(parent.data_ptr() + 2 * (off + c0), self.H * self.W * sw, self.W * sw, sw, c1 - c0, 0)

    def stage(self):
        """Device copies laid out as the engine lays them out: [q_loc | q_ls] slices of the posterior output, [p_loc | p_ls | p_feat]
        of the prior output, everything a channel slice of a wider parent; outputs filled with a recognisable value."""
        Z, Cw = self.Z, self.C
        e = {}
        e["qout"] = self.put(torch.cat([self.q_loc, self.q_ls], 1))
        e["pout"] = self.put(torch.cat([self.p_loc, self.p_ls, self.p_feat], 1))
        e["h"], e["eps"] = self.put(self.h), self.put(self.eps)
        c8 = _ceil(self.ctx, 8)
        pa = torch.zeros(self.pa.shape[0], c8 + 8, dtype=torch.float16)  # zero padded to 8 channels (cpad), 8 spare channels behind
        pa[:, :self.ctx] = self.pa
        pa[:, c8:] = 7.0
        e["pa"] = pa.cuda()
        for n, c in (("z", Z), ("h_out", Cw), ("zf", max(self.Cf, 8))):
            e[n] = self.put(torch.full((self.P, c), 77.0, dtype=torch.float16))
        e["kl"] = torch.full((self.B * self.kl_stride,), -5.0, device="cuda")
        e["img_p"], e["img_f"] = _fwd_image(self.w_p, [Z, self.ctx]).cuda(), _fwd_image(self.w_f, [Z, Cw]).cuda()
        e["b_p"], e["b_f"] = self.b_p.cuda(), self.b_f.cuda()
        e["rng"] = torch.tensor([0x1234567, 40], dtype=torch.int64, device="cuda")
        return e

    def pa_view(self, e):
        L = _lib()
        t = e["pa"]
        sw, c8 = t.shape[1], _ceil(self.ctx, 8)
        if self.pa_const:
            return L.View(t.data_ptr(), sw, 0, 0, self.ctx, c8)
        return L.View(t.data_ptr(), self.H * self.W * sw, self.W * sw, sw, self.ctx, c8)

    def args(self, e):
        L = _lib()
        Z = self.Z
        t = L.LatentTailFwdArgs()
        t.dtype, t.n, t.h, t.w, t.z_dim, t.c, t.ctx = L.F16, self.B, self.H, self.W, Z, self.C, self.ctx
        t.kl_stride, t.stream_id, t.logt = self.kl_stride, self.stream_id, self.logt
        t.q_loc, t.q_ls = self.view(e["qout"], 0, Z), self.view(e["qout"], Z, 2 * Z)
        t.p_loc, t.p_ls, t.p_feat = self.view(e["pout"], 0, Z), self.view(e["pout"], Z, 2 * Z), self.view(e["pout"], 2 * Z, 2 * Z + self.C)
        t.h_in, t.pa = self.view(e["h"]), self.pa_view(e)
        t.eps = self.view(e["eps"]) if self.has_eps else L.NULL_VIEW
        t.z, t.h_out = self.view(e["z"]), self.view(e["h_out"])
        t.zf = self.view(e["zf"], 0, self.Cf) if self.Cf else L.NULL_VIEW
        t.img_p, t.img_f = e["img_p"].data_ptr(), (e["img_f"].data_ptr() if self.Cf else None)
        t.bias_p, t.bias_f = e["b_p"].data_ptr(), (e["b_f"].data_ptr() if self.Cf else None)
        t.rng, t.kl_part = e["rng"].data_ptr(), e["kl"].data_ptr()
        return t

    def three_launches(self, e, lib, st):
        """cgen_reparam_kl_fwd + cgen_conv2d x 2 into the output buffers of `e`."""
        L = _lib()
        t = self.args(e)
        lib.reparam_kl_fwd(L.F16, self.B, self.H, self.W, self.Z, t.q_loc, t.q_ls, t.p_loc, t.p_ls, t.eps, t.rng, self.stream_id,
                           self.logt, t.z, L.NULL_VIEW, t.kl_part, self.kl_stride, st)

        def conv(seg1, img, bias, out, res1, res2):
            a = L.ConvArgs()
            a.dtype, a.n, a.h, a.w, a.ks, a.nseg, a.act, a.dact = L.F16, self.B, self.H, self.W, 1, 2, L.ACT_NONE, L.ACT_NONE
            a.seg[0], a.seg[1], a.weight, a.bias, a.out = t.z, seg1, img, bias, out
            a.aux, a.res1, a.res2 = L.NULL_VIEW, res1, res2
            lib.conv2d(C.byref(a), st)

        conv(t.pa, t.img_p, t.bias_p, t.h_out, t.h_in, t.p_feat)
        if self.Cf:
            conv(t.p_feat, t.img_f, t.bias_f, t.zf, L.NULL_VIEW, L.NULL_VIEW)


INPUTS = ("qout", "pout", "h", "eps", "pa")
OUTPUTS = ("z", "h_out", "zf")
_bits = lambda x: x.view(torch.int16)


def _clone(e):
    return {k: ((v[0].clone(), v[1], v[2]) if isinstance(v, tuple) else v.clone()) for k, v in e.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_one_launch_equals_the_three_launches_bit_for_bit(shape, variant):
    L = _lib()
    lib = L.require_gpu()
    case = Case(shape, variant)
    e = case.stage()
    ref = _clone(e)
    before = _clone(e)
    st = torch.cuda.current_stream().cuda_stream
    case.three_launches(ref, lib, st)
    t = case.args(e)
    assert lib.latent_tail_fwd_supported(C.byref(t)) == 1
    lib.latent_tail_fwd(C.byref(t), st)
    torch.cuda.synchronize()
    for n in OUTPUTS:
        got, want = _bits(e[n][0]), _bits(ref[n][0])
        assert torch.equal(got, want), (n, int((got != want).sum()), got.numel())
        parent, off, c = e[n]
        c = case.Cf if n == "zf" else c
        assert torch.isfinite(parent[:, off:off + c].float()).all(), n
        if c:  # (written at all: the fill value is gone)
            assert not (parent[:, off:off + c] == 77.0).all(), n
        # the channels next to the slice keep their bits
        assert torch.equal(_bits(parent[:, :off]), _bits(before[n][0][:, :off])) and torch.equal(_bits(parent[:, off + c:]), _bits(before[n][0][:, off + c:])), n
    assert torch.equal(e["kl"].view(torch.int32), ref["kl"].view(torch.int32)), (e["kl"] - ref["kl"]).abs().max().item()
    k = e["kl"].view(case.B, case.kl_stride)
    assert torch.isfinite(k[:, :case.chunks]).all() and (k[:, case.chunks:] == -5.0).all()
    for n in INPUTS:
        got = e[n][0] if isinstance(e[n], tuple) else e[n]
        was = before[n][0] if isinstance(before[n], tuple) else before[n]
        assert torch.equal(_bits(got), _bits(was)), n


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 24, 24, 128, 16), (3, 48, 48, 64, 16)], ids=["conv_smallp", "conv_px"])
def test_against_f64(shape):
    L = _lib()
    lib = L.require_gpu()
    assert not lib.h16_is_bf16  # (the bounds are binary16's)
    case = Case(shape, "eps-pamat-ctx20-cf_narrow")
    e = case.stage()
    t = case.args(e)
    assert lib.latent_tail_fwd_supported(C.byref(t)) == 1
    lib.latent_tail_fwd(C.byref(t), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    d = lambda x: x.double()
    Z, Cw, Cf = case.Z, case.C, case.Cf
    sl = lambda n, c: e[n][0][:, e[n][1]:e[n][1] + c].cpu().double()
    z_dev, h_dev, zf_dev = sl("z", Z), sl("h_out", Cw), sl("zf", Cf)
    # ---- z: one binary16 rounding
    sq = torch.exp(d(case.q_ls) + case.logt)
    z = d(case.q_loc) + sq * d(case.eps)
    a = d(case.q_loc).abs() + (sq * d(case.eps)).abs()
    err, bound = (z_dev - z).abs(), 2.0 ** -10 * z.abs() + 2.0 ** -22 * a + 2.0 ** -24
    print("z: worst error / bound = %.3f" % (err / bound).max().item())
    assert (err <= bound).all()
    # ---- the two GEMMs over the stored z
    pa = d(case.pa).repeat_interleave(case.H * case.W, 0) if case.pa_const else d(case.pa)
    for name, got, x, w, b, res in (("h_out", h_dev, torch.cat([z_dev, pa], 1), d(case.w_p), d(case.b_p), (d(case.h), d(case.p_feat))),
                                    ("zf", zf_dev, torch.cat([z_dev, d(case.p_feat)], 1), d(case.w_f), d(case.b_f), ())):
        v, a = x @ w.t() + b, x.abs() @ w.abs().t() + b.abs()
        for r in res:
            v, a = v + r, a + r.abs()
        K = x.shape[1] + 1 + len(res)
        err, bound = (got - v).abs(), 2.0 ** -10 * v.abs() + (K + 16) * 2.0 ** -24 * a + 2.0 ** -24
        print("%s: worst error / bound = %.3f" % (name, (err / bound).max().item()))
        assert torch.isfinite(got).all() and (err <= bound).all(), (name, int((err > bound).sum()))
    # ---- KL partials
    q, pp, dd = d(case.q_ls) + case.logt, d(case.p_ls) + case.logt, d(case.q_loc) - d(case.p_loc)
    quad = 0.5 * (torch.exp(2 * q) + dd * dd) / torch.exp(2 * pp)
    term, aterm = (-0.5 + pp - q + quad).view(case.B, -1), (0.5 + pp.abs() + q.abs() + quad).view(case.B, -1)
    kl = e["kl"].view(case.B, case.kl_stride).cpu().double()
    for c in range(case.chunks):
        v, a = term[:, c * LAT_CHUNK:(c + 1) * LAT_CHUNK].sum(1), aterm[:, c * LAT_CHUNK:(c + 1) * LAT_CHUNK].sum(1)
        n = min(LAT_CHUNK, term.shape[1] - c * LAT_CHUNK)
        assert ((kl[:, c] - v).abs() <= (n + 32) * 2.0 ** -24 * a).all(), c


def _declined():
    """(label, args, keep-alive, wanted answer) of calls; pointers are made-up addresses with the wanted alignment (never dereferenced:
    the entry point answers before it would launch)."""
    L = _lib()
    out = []

    def make(shape=(2, 12, 12, 64), dtype=None, mutate=None):
        B, H, W, Cw = shape
        Z, ctx = 16, 4
        t = L.LatentTailFwdArgs()
        t.dtype, t.n, t.h, t.w, t.z_dim, t.c, t.ctx = (L.F16 if dtype is None else dtype), B, H, W, Z, Cw, ctx
        t.kl_stride, t.stream_id, t.logt = 8, 1, 0.0
        base = [1 << 20]

        def view(c, sw=None):
            sw = c + 16 if sw is None else sw
            p = base[0]
            base[0] += _ceil(B * H * W * sw * 2 + 64, 256)
            return L.View(p, H * W * sw, W * sw, sw, c, 0)

        t.q_loc, t.q_ls, t.p_loc, t.p_ls, t.p_feat, t.h_in = view(Z), view(Z), view(Z), view(Z), view(Cw), view(Cw)
        t.pa = L.View(base[0], 8, 0, 0, ctx, 8)
        base[0] += 4096
        t.eps, t.z, t.h_out, t.zf = L.NULL_VIEW, view(Z), view(Cw), view(Cw)
        t.img_p, t.img_f, t.bias_p, t.bias_f, t.rng, t.kl_part = (base[0] + 256 * i for i in range(6))
        if mutate:
            mutate(t)
        return t

    out.append(("served", make(), 1))
    out.append(("f32", make(dtype=L.F32), 0))
    out.append(("C=16", make(shape=(2, 12, 12, 16)), 0))
    out.append(("C=512", make(shape=(3, 1, 1, 512)), 0))
    out.append(("a remainder plane on h", make(mutate=lambda t: setattr(t, "h_in_rem", 1 << 16)), 0))

    def off_by_8(t):
        v = t.h_in
        t.h_in = L.View(v.p + 8, v.sn, v.sh, v.sw, v.c, 0)

    out.append(("pointer off by 8 bytes", make(mutate=off_by_8), 0))

    def bad_row_stride(t):
        v = t.p_feat
        t.p_feat = L.View(v.p, v.sn, v.sh + 8, v.sw, v.c, 0)

    out.append(("sh != w * sw", make(mutate=bad_row_stride), 0))
    out.append(("ctx = 52: three K-steps", make(mutate=lambda t: (setattr(t, "ctx", 52), setattr(t, "pa", L.View(t.pa.p, 56, 0, 0, 52, 56)))), 0))
    return out


def test_supported_answers_without_a_gpu_and_declined_calls_return_the_error_code():
    lib = _lib().load()
    for label, t, want in _declined():
        assert lib.latent_tail_fwd_supported(C.byref(t)) == want, label
        if not want:  # the entry point answers with its error code before it would launch anything
            assert lib._raw_cgen_latent_tail_fwd(C.byref(t), None) == EUNSUPPORTED, label
            assert b"cgen_latent_tail_fwd" in lib.cdll.cgen_last_error()


# ----------------------------------------------------------------------------- model level
def _small_hp(**over):
    from causal_gen_amd.hps import setup_hparams

    return setup_hparams("ukbb192", input_res=24, enc_arch="24b1d2,12b1d2,6b1d6,1b1", dec_arch="1b1,6b2,12b2,24b2",
                         widths=[32, 64, 96, 128], z_max_res=24, z_dim=16, bs=3, **over)


def _one_pass(monkeypatch, knob, **over):
    monkeypatch.setenv("CGEN_LAT_TAIL_FWD", knob)
    hp = _small_hp(**over)
    m = _small_model(hp)
    x, pa = _batch(hp, 3)
    eng = m.engine()
    _seed(eng)
    l0 = eng.launches
    out = m(x, pa, beta=2.0)
    fwd_launches, fwd_tails = eng.launches - l0, eng.lat_tails_fwd
    out["elbo"].backward()
    torch.cuda.synchronize()
    vals = {k: out[k].detach().cpu().clone() for k in ("elbo", "nll", "kl")}
    grads = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters() if p.grad is not None}
    _seed(eng)
    with torch.no_grad():
        zs = [z.detach().cpu().clone() for z in m.eval().abduct(x, pa)]
    return vals, grads, zs, fwd_launches, fwd_tails


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "free_bits"])
def test_model_one_launch_against_three(monkeypatch, mode):
    """ELBO, NLL, KL, every collected z and every parameter gradient keep their bits; the forward launch count drops by 2 per served
    layer with z_feat_proj and by 1 for the last layer, which has none (all seven stochastic layers are served: 1x1, and two each at
    6x6, 12x12 and 24x24, widths 32 .. 128)."""
    _lib().require_gpu()
    over = {"plain": {}, "free_bits": {"kl_free_bits": 0.5}}[mode]
    v1, g1, z1, n1, t1 = _one_pass(monkeypatch, "1", **dict(over))
    v0, g0, z0, n0, t0 = _one_pass(monkeypatch, "0", **dict(over))
    assert t0 == 0 and t1 == 7, (t0, t1)
    print("forward launches: three-launch path %d, fused %d" % (n0, n1))
    assert n0 - n1 == 2 * 6 + 1, (n0, n1)
    assert len(z1) == len(z0) == 7
    for a, b in zip(z1, z0):
        assert torch.equal(a, b)
    _same((v1, g1), (v0, g0))


@pytest.mark.gpu
def test_train_step_graph_replay_equals_eager_on_the_fused_path(monkeypatch):
    from causal_gen_amd.train import TrainStep

    _lib().require_gpu()
    monkeypatch.setenv("CGEN_LAT_TAIL_FWD", "1")
    outs = []
    for use_graph in (False, True):
        hp = _small_hp(lr=2e-3, lr_warmup_steps=2)
        m = _small_model(hp)
        x, pa = _batch(hp, 3)
        torch.manual_seed(123)
        ts = TrainStep(m, SimpleNamespace(**vars(hp)), ema=True, use_graph=use_graph)
        for _ in range(3):
            o = ts.step(x, pa)
        torch.cuda.synchronize()
        assert m.engine().lat_tails_fwd == 7
        outs.append(([float(v) for v in o.cpu()], {k: v.clone() for k, v in m.state_dict().items()}))
    (o0, s0), (o1, s1) = outs
    assert o0 == o1, (o0, o1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
