"""The latent tail of a DETERMINISTIC decoder layer (z = p_loc) as one launch each way: cgen_latent_tail_fwd / cgen_latent_tail_bwd
called without q_loc / q_ls (csrc/latent_tail.hip), Engine.latent_tail_fwd without `q_loc` / _bw_latent_tail without `r`, CGEN_LAT_TAIL_DET.

Everything is compared bit for bit against the separate launches the fused ones stand for:
  forward   cgen_conv2d (z_proj over [p_loc | pa], res1 = h, res2 = p_feat) and cgen_conv2d (z_feat_proj over [p_loc | p_feat]);
  backward  z_feat_proj's two data gradients (stores into grad(p_loc), grad(p_feat)), the residual's copy of g_h landing on
            grad(p_feat) (cgen_axpby, accumulating behind z_feat_proj), z_proj's data gradient (accumulating into grad(p_loc)) and the
            zero fill of the p_ls channels -- the order Engine.backward issues them in for such a layer.

Kernel level, through the C ABI.  Every tensor lives in ONE device buffer filled with a byte pattern, between two guard bands; after the
calls every byte outside the written views -- bands, neighbouring channels, inputs -- still has its value.  Shapes: 2 x 56 x 56 (6 272
pixels: just over the small-image conv's 6 000) and 3 x 46 x 46 (6 348: no multiple of 64 or of a 256- / 512-pixel tile, partial last
tiles in every sample).  Model level: a small f16 HVAE whose two 64 x 64 layers are deterministic, CGEN_LAT_TAIL_DET=1 against =0."""
import ctypes as C
import itertools
import zlib
from types import SimpleNamespace

import pytest
import torch

from latent_tail_cases import _batch, _ceil, _dgrad_image, _fwd_image, _lib, _same, _seed, _small_model

EUNSUPPORTED = -3
SHAPES = [(2, 56, 56), (3, 46, 46)]
# (C, Z): up to 64 channels the backward runs as one workgroup row, above as two; 160 takes the widest forward and backward instances
WIDTHS = [(32, 16), (64, 16), (32, 8), (64, 8), (96, 16), (160, 16)]
CTX = {"ctx4const": (4, True), "ctx6mat": (6, False)}  # stride-0 parents zero padded to 8 | materialised parents
GUARD, PATTERN = 512, 0x5B
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


class Arena:
    """One device buffer full of PATTERN; every allocation sits between two guard bands of it."""

    def __init__(self, nbytes):
        self.buf = torch.full((nbytes,), PATTERN, dtype=torch.uint8, device="cuda")
        self.top, self.live = 0, []

    def put(self, t):
        """A copy of the CPU tensor `t` (any dtype, 2-D or 1-D) inside the buffer."""
        raw = t.contiguous().view(-1).view(torch.uint8)
        o = _ceil(self.top + GUARD, 256)
        self.top = o + raw.numel()
        assert self.top + GUARD <= self.buf.numel()
        self.buf[o:self.top] = raw.cuda()
        self.live.append((o, raw.numel()))
        return self.buf[o:self.top].view(t.dtype).view(t.shape)

    def outside_is_untouched(self):
        mask = torch.ones(self.buf.numel(), dtype=torch.bool, device="cuda")
        for o, n in self.live:
            mask[o:o + n] = False
        return bool((self.buf[mask] == PATTERN).all())


class Case:
    """The tensors of one layer.  pout = [p_loc Z | p_ls Z | p_feat C] is a tensor of exactly 2Z + C channels (its slices are the
    views); h, h', zf, g_h, g_f and grad(pout) are channel slices [8, 8 + c) of parents 16 channels wider."""

    def __init__(self, shape, width, ctx="ctx4const", feat=True):
        (self.B, self.H, self.W), (self.C, self.Z) = shape, width
        self.ctx, self.pa_const = CTX[ctx]
        self.feat = feat
        B, H, W, Cw, Z = self.B, self.H, self.W, self.C, self.Z
        P = self.P = B * H * W
        g = torch.Generator().manual_seed(zlib.crc32(repr((shape, width, ctx, feat)).encode()))
        rn = lambda *s: torch.randn(*s, generator=g)
        mag = lambda *s: rn(*s) * torch.pow(10.0, torch.rand(*s, generator=g) * 2.0 - 2.0)  # gradients O(1e-2 .. 1)
        wide = lambda t, fill: torch.cat([torch.full((P, 8), fill), t.float(), torch.full((P, 8), fill)], 1).half()
        w_p, w_f = (rn(Cw, Z + self.ctx) * 0.2).half(), (rn(Cw, Z + Cw) * 0.1).half()
        pa = rn(B, self.ctx)
        pa = pa if self.pa_const else pa.repeat_interleave(H * W, 0) + 0.25 * rn(P, self.ctx)
        pa8 = torch.zeros(pa.shape[0], 16)  # zero padded to 8 channels (cpad), 8 spare channels behind
        pa8[:, :self.ctx], pa8[:, 8:] = pa, 7.0
        nan = float("nan")
        cpu = dict(pout=torch.cat([rn(P, Z), torch.rand(P, Z, generator=g) * 3 - 2, rn(P, Cw)], 1).half(), h=wide(rn(P, Cw) * 3.0, 5.0),
                   pa=pa8.half(), g_h=wide(mag(P, Cw), 3.0), g_f=wide(mag(P, Cw), 3.0),
                   img_p=_fwd_image(w_p, [Z, self.ctx]), img_f=_fwd_image(w_f, [Z, Cw]), b_p=rn(Cw) * 0.5, b_f=rn(Cw) * 0.5,
                   img_pz=_dgrad_image(w_p, 0, Z), img_fz=_dgrad_image(w_f, 0, Z), img_fp=_dgrad_image(w_f, Z, Cw))
        for side in ("one", "sep"):  # outputs of the one launch | of the separate launches: same layout, same fill
            cpu["h_out_" + side], cpu["zf_" + side] = wide(torch.full((P, Cw), 77.0), 77.0), wide(torch.full((P, Cw), 77.0), 77.0)
            cpu["gp_" + side] = wide(torch.full((P, 2 * Z + Cw), nan), 9.0)
        self.arena = Arena(sum(t.numel() * t.element_size() + GUARD + 256 for t in cpu.values()) + GUARD)
        self.t = {k: self.arena.put(v) for k, v in cpu.items()}
        self.inputs = {k: self.t[k].clone() for k in ("pout", "h", "pa", "g_h", "g_f")}

    def view(self, name, c0, c1, off=8):
        """Channels [c0, c1) of tensor `name` (`off`: where its payload starts inside its parent)."""
        t = self.t[name]
        sw = t.shape[1]
        return _lib().View(t.data_ptr() + 2 * (off + c0), self.H * self.W * sw, self.W * sw, sw, c1 - c0, 0)

    def pa_view(self):
        t = self.t["pa"]
        if self.pa_const:
            return _lib().View(t.data_ptr(), 16, 0, 0, self.ctx, 8)
        return _lib().View(t.data_ptr(), self.H * self.W * 16, self.W * 16, 16, self.ctx, 8)

    def slices(self):
        Z, Cw = self.Z, self.C
        return self.view("pout", 0, Z, 0), self.view("pout", 2 * Z, 2 * Z + Cw, 0)  # p_loc, p_feat

    # ---- forward
    def fwd_args(self, side="one"):
        L = _lib()
        a = L.LatentTailFwdArgs()
        a.dtype, a.n, a.h, a.w, a.z_dim, a.c, a.ctx = L.F16, self.B, self.H, self.W, self.Z, self.C, self.ctx
        a.p_loc, a.p_feat = self.slices()
        a.h_in, a.pa = self.view("h", 0, self.C), self.pa_view()
        a.q_loc = a.q_ls = a.p_ls = a.eps = a.z = L.NULL_VIEW
        a.h_out = self.view("h_out_" + side, 0, self.C)
        a.zf = self.view("zf_" + side, 0, self.C) if self.feat else L.NULL_VIEW
        a.img_p, a.img_f = self.t["img_p"].data_ptr(), (self.t["img_f"].data_ptr() if self.feat else None)
        a.bias_p, a.bias_f = self.t["b_p"].data_ptr(), (self.t["b_f"].data_ptr() if self.feat else None)
        return a

    def fwd_separate(self, lib, st):
        L = _lib()
        t = self.fwd_args("sep")

        def conv(seg1, img, bias, out, res1, res2):
            a = L.ConvArgs()
            a.dtype, a.n, a.h, a.w, a.ks, a.nseg, a.act, a.dact = L.F16, self.B, self.H, self.W, 1, 2, L.ACT_NONE, L.ACT_NONE
            a.seg[0], a.seg[1], a.weight, a.bias, a.out = t.p_loc, seg1, img, bias, out
            a.aux, a.res1, a.res2 = L.NULL_VIEW, res1, res2
            lib.conv2d(C.byref(a), st)

        conv(t.pa, t.img_p, t.bias_p, t.h_out, t.h_in, t.p_feat)
        if self.feat:
            conv(t.p_feat, t.img_f, t.bias_f, t.zf, L.NULL_VIEW, L.NULL_VIEW)

    # ---- backward
    def bwd_args(self, side="one"):
        L = _lib()
        a = L.LatentTailArgs()
        a.dtype, a.n, a.h, a.w, a.z_dim, a.c, a.parity = L.F16, self.B, self.H, self.W, self.Z, self.C, 1
        a.g_h = self.view("g_h", 0, self.C)
        a.g_f = self.view("g_f", 0, self.C) if self.feat else L.NULL_VIEW
        a.gz_in = a.q_loc = a.q_ls = a.p_loc = a.p_ls = a.z = a.out_q = L.NULL_VIEW
        a.out_p = self.view("gp_" + side, 0, 2 * self.Z + self.C)
        a.img_pz = self.t["img_pz"].data_ptr()
        if self.feat:
            a.img_fz, a.img_fp = self.t["img_fz"].data_ptr(), self.t["img_fp"].data_ptr()
        return a

    def bwd_separate(self, lib, st):
        L = _lib()
        Z, Cw = self.Z, self.C
        g_h, g_f = self.view("g_h", 0, Cw), self.view("g_f", 0, Cw)
        gl, gs, gf = self.view("gp_sep", 0, Z), self.view("gp_sep", Z, 2 * Z), self.view("gp_sep", 2 * Z, 2 * Z + Cw)

        def dgrad(seg, img, out, acc):
            a = L.ConvArgs()
            a.dtype, a.n, a.h, a.w, a.ks, a.nseg, a.act, a.dact = L.F16, self.B, self.H, self.W, 1, 1, L.ACT_NONE, L.ACT_NONE
            a.seg[0], a.weight, a.bias, a.out = seg, self.t[img].data_ptr(), None, out
            a.aux, a.res1, a.res2 = L.NULL_VIEW, (out if acc else L.NULL_VIEW), L.NULL_VIEW
            lib.conv2d(C.byref(a), st)

        if self.feat:
            dgrad(g_f, "img_fz", gl, False)
            dgrad(g_f, "img_fp", gf, False)
        lib.axpby(L.F16, self.B, self.H, self.W, g_h, gf, 1.0, 1.0, 1 << 30, 1 if self.feat else 0, st)  # the rider, landed
        dgrad(g_h, "img_pz", gl, self.feat)
        lib.axpby(L.F16, self.B, self.H, self.W, L.NULL_VIEW, gs, 0.0, 1.0, 1 << 30, 0, st)  # the fill of grad(p_ls)

    def check(self, names):
        """The one launch's outputs equal the separate launches' in every byte of their parents; nothing else has moved."""
        bits = lambda x: x.view(torch.int16)
        for n in names:
            got, want = bits(self.t[n + "_one"]), bits(self.t[n + "_sep"])
            assert torch.equal(got, want), (n, int((got != want).sum()), got.numel())
        for k, was in self.inputs.items():
            assert torch.equal(bits(self.t[k]), bits(was)), k
        assert self.arena.outside_is_untouched(), "a guard band was written"


@pytest.mark.gpu
@pytest.mark.parametrize("feat", [True, False], ids=["zfeat", "last"])
@pytest.mark.parametrize("ctx", list(CTX))
@pytest.mark.parametrize("width", WIDTHS, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_forward_equals_the_two_convs_bit_for_bit(shape, width, ctx, feat):
    lib = _lib().require_gpu()
    case = Case(shape, width, ctx, feat)
    st = torch.cuda.current_stream().cuda_stream
    case.fwd_separate(lib, st)
    a = case.fwd_args()
    assert lib.latent_tail_fwd_supported(C.byref(a)) == 1
    lib.latent_tail_fwd(C.byref(a), st)
    torch.cuda.synchronize()
    case.check(["h_out", "zf"])
    h2 = case.t["h_out_one"][:, 8:8 + case.C]
    assert torch.isfinite(h2.float()).all() and not (h2 == 77.0).all()
    zf = case.t["zf_one"][:, 8:8 + case.C]
    assert bool((zf == 77.0).all()) != feat  # (written exactly when the layer has a z_feat_proj)


@pytest.mark.gpu
@pytest.mark.parametrize("feat", [True, False], ids=["zfeat", "last"])
@pytest.mark.parametrize("width", WIDTHS, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_backward_equals_the_launches_bit_for_bit(shape, width, feat):
    lib = _lib().require_gpu()
    case = Case(shape, width, feat=feat)
    st = torch.cuda.current_stream().cuda_stream
    case.bwd_separate(lib, st)
    a = case.bwd_args()
    assert lib.latent_tail_bwd_supported(C.byref(a)) == 1
    lib.latent_tail_bwd(C.byref(a), st)
    torch.cuda.synchronize()
    case.check(["gp"])
    Z, Cw = case.Z, case.C
    gp = case.t["gp_one"][:, 8:8 + 2 * Z + Cw]
    assert torch.isfinite(gp.float()).all()  # (the NaN fill is gone: every channel of the pixel was written)
    assert bool((gp[:, Z:2 * Z].view(torch.int16) == 0).all())  # grad(p_ls): +0
    if not feat:  # without z_feat_proj grad(p_feat) is g_h's bits
        assert torch.equal(gp[:, 2 * Z:].view(torch.int16), case.t["g_h"][:, 8:8 + Cw].view(torch.int16))


def _declined(dev):
    """(label, direction, args, keep-alive) the kernels must decline; pointers come from real tensors (never dereferenced)."""
    L = _lib()

    def make(shape=(2, 56, 56), width=(32, 16)):
        case = Case.__new__(Case)
        (case.B, case.H, case.W), (case.C, case.Z) = shape, width
        case.ctx, case.pa_const, case.feat = 4, True, True
        P, Cw, Z = case.B * case.H * case.W, case.C, case.Z
        z16 = lambda r, c: torch.zeros(r, c, dtype=torch.float16, device=dev)
        case.t = dict(pout=z16(P, 2 * Z + Cw), pa=z16(case.B, 16), img_p=z16(64, 64), img_f=z16(64, 128), img_pz=z16(16, 128),
                      img_fz=z16(16, 128), img_fp=z16(64, 128), b_p=torch.zeros(Cw, device=dev), b_f=torch.zeros(Cw, device=dev))
        for n in ("h", "g_h", "g_f", "h_out_one", "zf_one"):
            case.t[n] = z16(P, Cw + 16)
        case.t["gp_one"] = z16(P, 2 * Z + Cw + 16)
        return case

    out = []
    ok = make()
    out += [("served", "fwd", ok.fwd_args(), ok, 1), ("served", "bwd", ok.bwd_args(), ok, 1)]
    for label, shape in (("P = 6000", (2, 50, 60)), ("a side below 5", (4, 4, 400))):
        c = make(shape)
        out += [(label, "fwd", c.fwd_args(), c, 0), (label, "bwd", c.bwd_args(), c, 0)]
    c = make()
    f, b = c.fwd_args(), c.bwd_args()
    f.h_in = L.View(f.h_in.p + 8, f.h_in.sn, f.h_in.sh, f.h_in.sw, f.h_in.c, 0)
    b.out_p = L.View(b.out_p.p + 8, b.out_p.sn, b.out_p.sh, b.out_p.sw, b.out_p.c, 0)
    out += [("pointer off by 8 bytes", "fwd", f, c, 0), ("pointer off by 8 bytes", "bwd", b, c, 0)]
    f = c.fwd_args()
    f.h_in_rem = 1 << 20
    out.append(("remainder plane", "fwd", f, c, 0))
    b = c.bwd_args()
    b.acc_p = 1
    out.append(("grad(pout) holds a value", "bwd", b, c, 0))  # (the kernel does not accumulate: a refusal, not other bits)
    b = c.bwd_args()
    b.out_q = b.out_p
    out.append(("a reparam view without q_loc", "bwd", b, c, 0))
    return out


def _check_declined(dev, monkeypatch):
    lib = _lib().load()
    sup = {"fwd": lib.latent_tail_fwd_supported, "bwd": lib.latent_tail_bwd_supported}
    raw = {"fwd": lib._raw_cgen_latent_tail_fwd, "bwd": lib._raw_cgen_latent_tail_bwd}
    cases = _declined(dev)
    for label, d, a, keep, want in cases:
        assert sup[d](C.byref(a)) == want, (label, d)
        if not want:  # the entry point answers with its error code before it would launch anything
            assert raw[d](C.byref(a), None) == EUNSUPPORTED, (label, d)
    monkeypatch.setenv("CGEN_CONV_NO_PX", "1")  # a conv dispatch knob: the convs' kernel is no longer known from the shape
    for label, d, a, keep, want in cases[:2]:
        assert sup[d](C.byref(a)) == 0, ("dispatch knob", d)


def test_supported_answers_without_a_gpu(monkeypatch):
    _check_declined("cpu", monkeypatch)


@pytest.mark.gpu
def test_declined_cases_return_the_error_code(monkeypatch):
    _lib().require_gpu()
    _check_declined("cuda", monkeypatch)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- model level
def _small_hp(**over):
    from causal_gen_amd.hps import setup_hparams

    # 64 x 64 input, z_max_res 32: the two 64 x 64 decoder layers are deterministic (C = 32, Z = 16; 2 x 64 x 64 = 8 192 pixels)
    return setup_hparams("ukbb192", input_res=64, enc_arch="64b1d2,32b1d4,8b1d8,1b1", dec_arch="1b1,8b1,32b1,64b2",
                         widths=[32, 32, 64, 64], z_max_res=32, z_dim=16, bs=2, **over)


def _one_pass(monkeypatch, knob, B=2, **env):
    monkeypatch.setenv("CGEN_LAT_TAIL_DET", knob)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    hp = _small_hp()
    m = _small_model(hp)
    x, pa = _batch(hp, B)
    eng = m.engine()
    _seed(eng)
    l0 = eng.launches
    out = m(x, pa, beta=2.0)
    out["elbo"].backward()
    torch.cuda.synchronize()
    for k in env:
        monkeypatch.delenv(k)
    vals = {k: out[k].detach().cpu().clone() for k in ("elbo", "nll", "kl")}
    grads = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters() if p.grad is not None}
    counts = SimpleNamespace(launches=eng.launches - l0, pairs=eng._conv.pairs, det=eng.lat_tails_det, det_fwd=eng.lat_tails_det_fwd,
                             sto=eng.lat_tails, sto_fwd=eng.lat_tails_fwd)
    return vals, grads, counts


@pytest.mark.gpu
def test_model_one_launch_each_way_against_the_separate_launches(monkeypatch):
    """ELBO, NLL, KL and every parameter gradient keep their bits.  Launches, as the parent's trace lists them for such a layer: the
    layer with z_feat_proj loses one forward (two convs -> one) and four backward (two + one data gradients, the landed rider and the
    zero fill -> one); the last layer none forward (its z_proj was one launch) and two backward (data gradient, rider, fill -> one).
    Seven in all.  The stochastic layers' fused tails are counted as before."""
    _lib().require_gpu()
    v1, g1, c1 = _one_pass(monkeypatch, "1")
    v0, g0, c0 = _one_pass(monkeypatch, "0")
    print("forward + backward launches: separate %d (%d pair launches), fused %d (%d)" % (c0.launches, c0.pairs, c1.launches, c1.pairs))
    assert (c0.det, c0.det_fwd, c1.det, c1.det_fwd) == (0, 0, 2, 2)
    assert (c1.sto, c1.sto_fwd) == (c0.sto, c0.sto_fwd) and c0.sto > 0
    assert (c0.launches + c0.pairs) - (c1.launches + c1.pairs) == 7, (c0.launches, c0.pairs, c1.launches, c1.pairs)
    _same((v1, g1), (v0, g0))
    assert any("z_feat_proj" in n for n in g1) and any("z_proj" in n for n in g1)


@pytest.mark.gpu
@pytest.mark.parametrize("why", ["few_pixels", "dispatch_knob", "remainder_planes"])
def test_model_declined_layers_run_the_separate_launches(monkeypatch, why):
    """What the kernels or the engine decline runs as before: no fused launch, the same launch count, the same bits.  4 096 pixels (one
    sample) are the small-image conv's; CGEN_CONV_NO_PX takes conv_px away from cgen_conv2d; CGEN_TRUNK_REM=2 gives h a remainder plane,
    which the FORWARD launch does not serve (the backward one never sees it: gradients have no remainder plane)."""
    _lib().require_gpu()
    kw = {"few_pixels": dict(B=1), "dispatch_knob": dict(CGEN_CONV_NO_PX="1"), "remainder_planes": dict(CGEN_TRUNK_REM="2")}[why]
    v1, g1, c1 = _one_pass(monkeypatch, "1", **kw)
    v0, g0, c0 = _one_pass(monkeypatch, "0", **kw)
    assert c1.det_fwd == 0
    if why != "remainder_planes":
        assert c1.det == 0 and c1.launches == c0.launches
    _same((v1, g1), (v0, g0))


@pytest.mark.gpu
def test_train_step_graph_replay_equals_eager_and_the_separate_launches(monkeypatch):
    from causal_gen_amd.train import TrainStep

    _lib().require_gpu()
    outs = []
    for knob, use_graph in (("1", False), ("1", True), ("0", True)):
        monkeypatch.setenv("CGEN_LAT_TAIL_DET", knob)
        hp = _small_hp(lr=2e-3, lr_warmup_steps=2)
        m = _small_model(hp)
        x, pa = _batch(hp, 2)
        torch.manual_seed(123)
        ts = TrainStep(m, SimpleNamespace(**vars(hp)), ema=True, use_graph=use_graph)
        for _ in range(3):
            o = ts.step(x, pa)
        torch.cuda.synchronize()
        assert m.engine().lat_tails_det == (2 if knob == "1" else 0)
        outs.append(([float(v) for v in o.cpu()], {k: v.clone() for k, v in m.state_dict().items()}))
    for o1, s1 in outs[1:]:
        assert outs[0][0] == o1, (outs[0][0], o1)
        for k in s1:
            assert torch.equal(outs[0][1][k], s1[k]), k
