"""The backward latent tail of a stochastic decoder layer as one launch (csrc/latent_tail.hip, cgen_latent_tail_bwd).

Kernel level, through the C ABI on views over torch tensors, against an f64 torch reference on the CPU computed from the
binary16-rounded inputs and the binary16-rounded weights (the values the kernel multiplies).  Per output element with exact value v
and A = the f64 sum of the absolute values of its terms:

    |out - v| <= 2^-10 |v| + (K + 16) 2^-24 A + 2^-24,   K = 2 C

(one binary16 rounding with a factor of two to spare, the worst-case bound of an f32 sum of K + 16 terms, the binary16 subnormal
step).  Every element is checked.  Outputs are channel slices of wider buffers, as the engine passes them; what the call must not
write -- the neighbouring channels, g_h, g_f -- is compared bit for bit after it.

That is the kernel's `parity = 0` arithmetic (one f32 sum, one rounding per output).  The engine's default is `parity = 1`: the same
launch reproducing the four launches it replaces bit for bit (each GEMM summed in their kernel's order, grad(z) and grad(p_feat)
rounded to binary16 where they store them), so that a training run computes what it computed before; that mode is held to exactly
that -- equal bits against cgen_conv2d x 3 + cgen_reparam_kl_bwd_rider through the C ABI, at shapes served by either of their kernels.

Model level: a small f16 HVAE whose layers the kernel serves (the golden fixtures are too narrow), CGEN_LAT_TAIL=1 against =0 and
against the f32 engine on the same weights and noise."""
import ctypes as C
import math
import zlib
from types import SimpleNamespace

import pytest
import torch

from latent_tail_cases import _batch, _ceil, _dgrad_image, _lib, _seed, _small_model

Z = 16
CTX = 4
SHAPES = [(3, 6, 6, 192), (2, 12, 12, 160), (2, 24, 24, 128), (1, 20, 24, 32), (2, 48, 48, 96)]
VARIANTS = ["plain", "no_gf", "gz_in", "acc", "chan_scale"]
EUNSUPPORTED = -3


class Case:
    """Inputs of one call on the CPU (binary16 values), the device copies inside wider parents, and the f64 reference."""

    def __init__(self, shape, variant, dev):
        B, H, W, Cw = shape
        self.shape, self.variant, self.dev = shape, variant, dev
        g = torch.Generator().manual_seed(zlib.crc32(repr((shape, variant)).encode()))
        P = B * H * W
        self.has_gf, self.has_gz, self.acc, self.chan = variant != "no_gf", variant == "gz_in", variant == "acc", variant == "chan_scale"
        rn = lambda *s: torch.randn(*s, generator=g)
        ru = lambda lo, hi, *s: torch.rand(*s, generator=g) * (hi - lo) + lo
        mag = lambda *s: rn(*s) * torch.pow(10.0, ru(-2.0, 0.0, *s))  # gradients O(1e-2 .. 1)
        h16 = lambda t: t.half()
        self.g_h, self.g_f = h16(mag(P, Cw)), h16(mag(P, Cw))
        self.gz_in = h16(mag(P, Z))
        self.q_loc, self.p_loc, self.z = h16(rn(P, Z)), h16(rn(P, Z)), h16(rn(P, Z))
        self.q_ls, self.p_ls = h16(ru(-2.0, 1.0, P, Z)), h16(ru(-2.0, 1.0, P, Z))
        self.w_f = rn(Cw, Z + Cw) * 0.1   # z_feat_proj: OI of a 1x1 conv over cat[z, p_feat]
        self.w_p = rn(Cw, Z + CTX) * 0.1  # z_proj: over cat[z, pa]
        self.prev_p, self.prev_q = h16(mag(P, 2 * Z + Cw)), h16(mag(P, 2 * Z))
        self.coef = ru(0.5, 2.0, B).float()
        self.chan_scale = ru(0.0, 1.0, Z).float()
        self.chan_scale[[1, 7, 12]] = 0.0
        self.logt = math.log(0.9)
        self.P, self.C = P, Cw

    # ---- device side: every tensor is a channel slice [off, off + c) of a parent with `pad` more channels on both sides
    def put(self, t, c_off=8, c_extra=16, fill=None):
        P, c = t.shape
        parent = torch.randn(P, c + c_extra, generator=torch.Generator().manual_seed(5)).half() if fill is None else torch.full((P, c + c_extra), fill).half()
        parent[:, c_off:c_off + c] = t
        return parent.to(self.dev), c_off, c

    def view(self, ent, c0=0, c1=None):
        L = _lib()
        parent, off, c = ent
        B, H, W, _ = self.shape
        c1 = c if c1 is None else c1
        sw = parent.shape[1]
        return L.View(parent.data_ptr() + 2 * (off + c0), H * W * sw, W * sw, sw, c1 - c0, 0)

    def reference(self):
        d = lambda t: t.double()
        wf, wp = d(self.w_f.half()), d(self.w_p.half())
        gh, gf = d(self.g_h), d(self.g_f)
        B, H, W, Cw = self.shape
        gz = gh @ wp[:, :Z]
        a_gz = gh.abs() @ wp[:, :Z].abs()
        gpf, a_pf = gh.clone(), gh.abs()
        if self.has_gf:
            gz = gz + gf @ wf[:, :Z]
            a_gz = a_gz + gf.abs() @ wf[:, :Z].abs()
            gpf = gpf + gf @ wf[:, Z:]
            a_pf = a_pf + gf.abs() @ wf[:, Z:].abs()
        if self.has_gz:
            gz = gz + d(self.gz_in)
            a_gz = a_gz + d(self.gz_in).abs()
        k = d(self.coef).repeat_interleave(H * W)[:, None].expand(-1, Z)
        if self.chan:
            k = k * d(self.chan_scale)[None, :]
        ql, qs, pl, ps, z = d(self.q_loc), d(self.q_ls) + self.logt, d(self.p_loc), d(self.p_ls) + self.logt, d(self.z)
        dd, e2q, ie2p = ql - pl, torch.exp(2 * qs), torch.exp(-2 * ps)
        t1 = k * dd * ie2p
        out_q = torch.cat([t1 + gz, k * (e2q * ie2p - 1) + gz * (z - ql)], 1)
        a_q = torch.cat([t1.abs() + a_gz, k.abs() * (e2q * ie2p + 1) + a_gz * (z - ql).abs()], 1)
        out_p = torch.cat([-t1, k * (1 - (e2q + dd * dd) * ie2p), gpf], 1)
        a_p = torch.cat([t1.abs(), k.abs() * (1 + (e2q + dd * dd) * ie2p), a_pf], 1)
        if self.acc:
            out_q, a_q = out_q + d(self.prev_q), a_q + d(self.prev_q).abs()
            out_p, a_p = out_p + d(self.prev_p), a_p + d(self.prev_p).abs()
        return out_p, a_p, out_q, a_q


def _args(case, dev_ents):
    L = _lib()
    B, H, W, Cw = case.shape
    e = dev_ents
    t = L.LatentTailArgs()
    t.dtype, t.n, t.h, t.w, t.z_dim, t.c = L.F16, B, H, W, Z, Cw
    t.coef_stride, t.acc_q, t.acc_p, t.logt, t.parity = 1, int(case.acc), int(case.acc), case.logt, 0
    t.g_h = case.view(e["g_h"])
    t.g_f = case.view(e["g_f"]) if case.has_gf else L.NULL_VIEW
    t.gz_in = case.view(e["gz_in"]) if case.has_gz else L.NULL_VIEW
    t.q_loc, t.q_ls = case.view(e["qout"], 0, Z), case.view(e["qout"], Z, 2 * Z)
    t.p_loc, t.p_ls = case.view(e["pout"], 0, Z), case.view(e["pout"], Z, 2 * Z)
    t.z = case.view(e["z"])
    t.out_p, t.out_q = case.view(e["out_p"]), case.view(e["out_q"])
    t.img_fz, t.img_fp, t.img_pz = e["img_fz"].data_ptr(), e["img_fp"].data_ptr(), e["img_pz"].data_ptr()
    t.coef = e["coef"].data_ptr()
    t.chan_scale = e["chan_scale"].data_ptr() if case.chan else None
    return t


def _stage(case):
    """Device copies: the forward tensors as the engine lays them out (q_loc | q_ls slices of the posterior output, p_loc | p_ls of
    the prior output), the outputs as slices of wider gradient buffers."""
    dev = case.dev
    e = {}
    for n in ("g_h", "g_f", "gz_in", "z"):
        e[n] = case.put(getattr(case, n))
    e["qout"] = case.put(torch.cat([case.q_loc, case.q_ls], 1))
    e["pout"] = case.put(torch.cat([case.p_loc, case.p_ls], 1), c_extra=16 + case.C)
    e["out_p"] = case.put(case.prev_p if case.acc else torch.full_like(case.prev_p, float("nan")))
    e["out_q"] = case.put(case.prev_q if case.acc else torch.full_like(case.prev_q, float("nan")))
    w16_f, w16_p = case.w_f.half(), case.w_p.half()
    e["img_fz"] = _dgrad_image(w16_f, 0, Z).to(dev)
    e["img_fp"] = _dgrad_image(w16_f, Z, case.C).to(dev)
    e["img_pz"] = _dgrad_image(w16_p, 0, Z).to(dev)
    e["coef"], e["chan_scale"] = case.coef.to(dev), case.chan_scale.to(dev)
    return e


_REF = {}


def _reference(shape, variant):
    key = (shape, variant)
    if key not in _REF:
        case = Case(shape, variant, "cpu")
        _REF[key] = (case, case.reference())
    return _REF[key]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_f64(shape, variant):
    L = _lib()
    lib = L.require_gpu()
    assert not lib.h16_is_bf16  # (the kernel and this bound are binary16's; a -DCGEN_H16_BF16 A/B build is not for this test)
    case, (rp, ap, rq, aq) = _reference(shape, variant)
    case.dev = "cuda"
    e = _stage(case)
    before = {n: e[n][0].clone() for n in ("g_h", "g_f", "gz_in", "z", "qout", "pout", "out_p", "out_q")}
    t = _args(case, e)
    assert lib.latent_tail_bwd_supported(C.byref(t)) == 1
    lib.latent_tail_bwd(C.byref(t), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    K = 2 * case.C
    for name, ref, a in (("out_p", rp, ap), ("out_q", rq, aq)):
        parent, off, c = e[name]
        got = parent[:, off:off + c].cpu().double()
        bound = 2.0 ** -10 * ref.abs() + (K + 16) * 2.0 ** -24 * a + 2.0 ** -24
        err = (got - ref).abs()
        worst = (err / bound).max().item()
        print("%s %s %s: worst error / bound = %.3f (max |err| %.3e)" % (shape, variant, name, worst, err.max().item()))
        assert torch.isfinite(got).all()
        assert (err <= bound).all(), (name, worst, int((err > bound).sum()))
        # the channels next to the slice keep their bits
        bits = lambda x: x.view(torch.int16)
        assert torch.equal(bits(parent[:, :off]), bits(before[name][:, :off])) and torch.equal(bits(parent[:, off + c:]), bits(before[name][:, off + c:])), name
    for n in ("g_h", "g_f", "gz_in", "z", "qout", "pout"):
        assert torch.equal(e[n][0].view(torch.int16), before[n].view(torch.int16)), n


PARITY_SHAPES = [(2, 24, 24, 128), (3, 48, 48, 64), (3, 6, 6, 192), (1, 20, 24, 32)]  # 6912 pixels: conv_px's order; the others conv_smallp's


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", PARITY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity_mode_equals_the_four_launches_bit_for_bit(shape, variant):
    L = _lib()
    lib = L.require_gpu()
    case = Case(shape, variant, "cuda")
    e = _stage(case)
    B, H, W, Cw = shape
    st = torch.cuda.current_stream().cuda_stream
    # ---- the four launches, on copies of the output parents and a grad(z) buffer of their own
    ref = {n: (e[n][0].clone(), e[n][1], e[n][2]) for n in ("out_p", "out_q")}
    gzbuf = case.put(case.gz_in if case.has_gz else torch.full_like(case.gz_in, float("nan")))
    gzv, pfv = case.view(gzbuf), case.view(ref["out_p"], 2 * Z, 2 * Z + Cw)

    def conv(seg, img, out, acc):
        a = L.ConvArgs()
        a.dtype, a.n, a.h, a.w, a.ks, a.nseg, a.act, a.dact = L.F16, B, H, W, 1, 1, L.ACT_NONE, L.ACT_NONE
        a.seg[0], a.weight, a.bias, a.out = seg, img.data_ptr(), None, out
        a.aux, a.res1, a.res2 = L.NULL_VIEW, (out if acc else L.NULL_VIEW), L.NULL_VIEW
        lib.conv2d(C.byref(a), st)

    if case.has_gf:
        conv(case.view(e["g_f"]), e["img_fz"], gzv, case.has_gz)
        conv(case.view(e["g_f"]), e["img_fp"], pfv, case.acc)
    conv(case.view(e["g_h"]), e["img_pz"], gzv, case.has_gf or case.has_gz)
    t = _args(case, e)
    lib.reparam_kl_bwd_rider(L.F16, B, H, W, Z, t.q_loc, t.q_ls, t.p_loc, t.p_ls, t.z, case.logt, gzv, t.coef, 1, t.chan_scale,
                             case.view(ref["out_q"], 0, Z), case.view(ref["out_q"], Z, 2 * Z), case.view(ref["out_p"], 0, Z),
                             case.view(ref["out_p"], Z, 2 * Z), int(case.acc), int(case.acc), case.view(e["g_h"]), pfv,
                             1 if (case.has_gf or case.acc) else 0, st)
    # ---- the one launch
    t.parity = 1
    assert lib.latent_tail_bwd_supported(C.byref(t)) == 1
    lib.latent_tail_bwd(C.byref(t), st)
    torch.cuda.synchronize()
    for n in ("out_p", "out_q"):
        got, want = e[n][0].view(torch.int16), ref[n][0].view(torch.int16)
        assert torch.equal(got, want), (n, int((got != want).sum()), got.numel())


def _declined(dev):
    """(label, args) of the calls the kernel must decline; pointers come from real tensors on `dev` (never dereferenced on the CPU)."""
    L = _lib()
    out = []

    def make(shape=(2, 12, 12, 64), mutate=None):
        case = Case.__new__(Case)
        B, H, W, Cw = shape
        case.shape, case.dev, case.C, case.P = shape, dev, Cw, B * H * W
        case.has_gf, case.has_gz, case.acc, case.chan, case.logt = True, False, False, False, 0.0
        P = case.P
        zeros = lambda c: torch.zeros(P, c, dtype=torch.float16)
        e = {n: case.put(zeros(c), fill=0.0) for n, c in (("g_h", Cw), ("g_f", Cw), ("gz_in", Z), ("z", Z), ("qout", 2 * Z), ("pout", 2 * Z),
                                                          ("out_p", 2 * Z + Cw), ("out_q", 2 * Z))}
        for n in ("img_fz", "img_fp", "img_pz"):
            e[n] = torch.zeros(_ceil(Cw, 16) * (_ceil(Cw, 32) + 32), dtype=torch.float16, device=dev)
        e["coef"], e["chan_scale"] = torch.ones(B, device=dev), torch.ones(Z, device=dev)
        t = _args(case, e)
        if mutate:
            mutate(t)
        return t, e

    ok = make()
    assert ok[0] is not None
    out.append(("served", ok, 1))
    out.append(("f32", make(mutate=lambda t: setattr(t, "dtype", L.F32)), 0))
    out.append(("C=20", make(shape=(2, 12, 12, 20)), 0))
    out.append(("C=512", make(shape=(3, 1, 1, 512)), 0))

    def bad_row_stride(t):
        v = t.g_h
        t.g_h = L.View(v.p, v.sn, v.sh + 8, v.sw, v.c, 0)

    out.append(("sh != w*sw", make(mutate=bad_row_stride), 0))

    def off_by_8(t):
        v = t.out_q
        t.out_q = L.View(v.p + 8, v.sn, v.sh, v.sw, v.c, 0)

    out.append(("pointer off by 8 bytes", make(mutate=off_by_8), 0))
    return out


def _check_declined(dev):
    L = _lib()
    lib = L.load()
    for label, (t, keep), want in _declined(dev):
        assert lib.latent_tail_bwd_supported(C.byref(t)) == want, label
        if not want:  # the entry point answers with its error code before it would launch anything
            assert lib._raw_cgen_latent_tail_bwd(C.byref(t), None) == EUNSUPPORTED, label
            assert b"cgen_latent_tail_bwd" in lib.cdll.cgen_last_error()


def test_supported_answers_without_a_gpu():
    _check_declined("cpu")


@pytest.mark.gpu
def test_declined_cases_return_the_error_code():
    _lib().require_gpu()
    _check_declined("cuda")
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- model level
def _small_hp(**over):
    from causal_gen_amd.hps import setup_hparams

    return setup_hparams("ukbb192", input_res=24, enc_arch="24b1d2,12b1d2,6b1d6,1b1", dec_arch="1b1,6b2,12b2,24b2",
                         widths=[32, 64, 96, 128], z_max_res=24, z_dim=16, bs=3, **over)


def _one_backward(monkeypatch, dtype, tail, exact="0", **over):
    monkeypatch.setenv("CGEN_LAT_TAIL", tail)
    monkeypatch.setenv("CGEN_LAT_TAIL_EXACT", exact)
    drop = over.pop("drop", None)
    hp = _small_hp(**over)
    m = _small_model(hp, dtype)
    if drop is not None:
        m.decoder.is_drop_cond = True
        m.decoder.drop_cond = lambda: drop
    x, pa = _batch(hp, 3)
    eng = m.engine()
    _seed(eng)
    l0 = eng.launches
    out = m(x, pa, beta=2.0)
    out["elbo"].backward()
    torch.cuda.synchronize()
    vals = {k: float(out[k]) for k in ("elbo", "nll", "kl")}
    grads = {n: p.grad.detach().double().cpu() for n, p in m.named_parameters() if p.grad is not None}
    return vals, grads, eng.launches - l0, eng.lat_tails, eng._conv.pairs


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "free_bits", "cond_dropout"])
def test_model_fused_tail_against_four_launches_and_f32(monkeypatch, mode):
    """Default arithmetic (parity): every parameter gradient has the bits of the four-launch path.  CGEN_LAT_TAIL_EXACT=1 (one rounding
    per output), the checks the issue sets: ELBO / NLL / KL keep their bits (the forward pass is untouched); the launch count drops by 3 per fused layer with z_feat_proj
    and by 1 for the last layer (none) -- counted in launches of the four-launch path as the issue lists them: where that path runs
    z_feat_proj's two data gradients as ONE pair launch (cgen_conv2d_pair, the small-image layers), the pair counts as the two
    launches it stands for; fusing may move a parameter gradient, but not away from the f32 engine's."""
    _lib().require_gpu()
    over = {"plain": {}, "free_bits": {"kl_free_bits": 0.5}, "cond_dropout": {"cond_prior": True, "drop": (0, 1)}}[mode]
    v1, g1, n1, tails, pairs1 = _one_backward(monkeypatch, "f16", "1", exact="1", **dict(over))
    v0, g0, n0, tails0, pairs0 = _one_backward(monkeypatch, "f16", "0", **dict(over))
    vp, gp, np_, tailsp, pairsp = _one_backward(monkeypatch, "f16", "1", **dict(over))  # the default arithmetic: the four launches' bits
    assert vp == v0 and (np_, tailsp, pairsp) == (n1, tails, pairs1)
    assert set(gp) == set(g0)
    for n in g0:
        assert torch.equal(gp[n], g0[n]), (n, float((gp[n] - g0[n]).abs().max()))
    _, g32, _, _, _ = _one_backward(monkeypatch, "f32", "1", **dict(over))
    assert v1 == v0, (v1, v0)
    n_feat, n_last = 6, 1  # seven stochastic layers (1x1, 2 x 6x6, 2 x 12x12, 2 x 24x24), the last one without z_feat_proj
    assert tails0 == 0 and tails == n_feat + n_last, (tails0, tails)
    print("launches: four-launch path %d (%d pair launches), fused %d (%d pair launches)" % (n0, pairs0, n1, pairs1))
    assert (n0 + pairs0) - (n1 + pairs1) == 3 * n_feat + n_last, (n0, pairs0, n1, pairs1)
    assert set(g1) == set(g0) == set(g32)
    for n, r in g32.items():
        den = float(r.norm())
        if den == 0:
            assert float(g1[n].norm()) == 0 and float(g0[n].norm()) == 0, n
            continue
        d1, d0, d10 = float((g1[n] - r).norm()) / den, float((g0[n] - r).norm()) / den, float((g1[n] - g0[n]).norm()) / den
        print("%-44s fused-f32 %.3e  four-f32 %.3e  fused-four %.3e" % (n, d1, d0, d10))
        assert math.isfinite(d1) and d1 <= d0 + d10, (n, d1, d0, d10)


@pytest.mark.gpu
def test_train_step_graph_replay_equals_eager_on_the_fused_path(monkeypatch):
    from causal_gen_amd.train import TrainStep

    _lib().require_gpu()
    monkeypatch.setenv("CGEN_LAT_TAIL", "1")
    outs = []
    for use_graph in (False, True):
        hp = _small_hp(lr=2e-3, lr_warmup_steps=2)
        m = _small_model(hp, "f16")
        x, pa = _batch(hp, 3)
        torch.manual_seed(123)
        ts = TrainStep(m, SimpleNamespace(**vars(hp)), ema=True, use_graph=use_graph)
        for _ in range(3):
            o = ts.step(x, pa)
        torch.cuda.synchronize()
        assert m.engine().lat_tails == 7
        outs.append(([float(v) for v in o.cpu()], {k: v.clone() for k, v in m.state_dict().items()}))
    (o0, s0), (o1, s1) = outs
    assert o0 == o1, (o0, o1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
