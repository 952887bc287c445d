"""Gradients through the DMoL decode (dmol.py:121-215) on the HIP path: the module-level mean / sample functions under autograd
(`cgen_dmol_decode_bwd`), the fused counterfactual step over two mixture-mean decodes (`cgen_cf_dmol_bwd`) and DSCM.forward
under autograd with a DmolNet head, each against torch autograd over the oracle in f64."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gpu_dscm import _dscm_case
from test_gpu_ops import _philox_words, _u01, make_engine

pytestmark = pytest.mark.gpu

MASKS = ["soft", "hard", "top1", "top3", "top9"]
EDGE = 1e-4


def _sel(l, mask):
    """Selection weights of dmol_ref.dmol_mean in f64 (and for top-k the kept set)."""
    lg = l[..., :10]
    if mask == "soft":
        return torch.softmax(lg, -1), torch.ones_like(lg, dtype=torch.bool)
    k = 1 if mask == "hard" else int(mask[-1])
    v = lg.sort(-1, descending=True)[0]
    keep = lg >= v[..., k - 1:k]
    if mask == "hard":
        return torch.nn.functional.one_hot(lg.argmax(-1), 10).double(), keep
    return torch.softmax(lg.masked_fill(~keep, -np.inf), -1), keep


def _chain(l, sel, nz=None, t=None):
    """Pre-clamp values of the three sequential RGB clamps and the raw mixed log-scales, f64."""
    rest = l[..., 10:].reshape(*l.shape[:-1], 3, 30)
    s_ = sel.unsqueeze(-2)
    mu = (rest[..., :10] * s_).sum(-1)
    s = (rest[..., 10:20] * s_).sum(-1)
    co = (torch.tanh(rest[..., 20:]) * s_).sum(-1)
    if nz is not None:
        ls = s.clamp(min=-7.0) + (0.0 if t is None else float(np.log(t)))
        mu = mu + ls.exp() * nz
    p0 = mu[..., 0]
    x0 = p0.clamp(-1, 1)
    p1 = mu[..., 1] + co[..., 0] * x0
    x1 = p1.clamp(-1, 1)
    p2 = mu[..., 2] + co[..., 1] * x0 + co[..., 2] * x1
    return torch.stack([p0, p1, p2], -1), s


def _draw(shape, g, ls_mu=-7.0):
    """Logits with a wide spread: means ~ +-2, log-scales around ls_mu (the -7 floor by default), coefficient
    pre-activations ~ +-3."""
    l = torch.empty(*shape, 100)
    l[..., :10] = torch.randn(*shape, 10, generator=g) * 2.0
    rest = torch.empty(*shape, 3, 30)
    rest[..., :10] = (torch.rand(*shape, 3, 10, generator=g) * 2 - 1) * 2.0
    rest[..., 10:20] = ls_mu + torch.randn(*shape, 3, 10, generator=g) * 1.5
    rest[..., 20:] = (torch.rand(*shape, 3, 10, generator=g) * 2 - 1) * 3.0
    l[..., 10:] = rest.reshape(*shape, 90)
    return l


def _ambiguous(l, mask, pre, s):
    """Pixels on a branch edge (within EDGE of a clamp end, of the -7 floor, or of a top-k / arg-max tie)."""
    bad = ((pre.abs() - 1).abs() < EDGE).any(-1) | ((s + 7).abs() < EDGE).any(-1)
    if mask != "soft":
        k = 1 if mask == "hard" else int(mask[-1])
        v = l[..., :10].sort(-1, descending=True)[0]
        bad |= (v[..., k - 1] - v[..., k]).abs() < EDGE
    return bad


def _mean_logits(mask, g, shape=(2, 8, 8), ls_mu=-7.0, dtype=torch.float32):
    """Logits as stored in `dtype` (returned as f32) with no pixel on a branch edge."""
    l = _draw(shape, g, ls_mu).to(dtype).float()
    for _ in range(50):
        l64 = l.double()
        sel, _ = _sel(l64, mask)
        pre, s = _chain(l64, sel)
        bad = _ambiguous(l64, mask, pre, s)
        if not bad.any():
            return l, pre, s
        l[bad] = _draw((int(bad.sum()),), g, ls_mu).to(dtype).float()
    raise AssertionError("could not draw unambiguous logits")


def _branches_hit(pre, s):
    for c in range(3):
        inside = pre[..., c].abs() <= 1
        assert inside.any() and (~inside).any(), f"clamp {c} must be hit on both sides"
    assert (s < -7).any() and (s > -7).any(), "the -7 floor must be hit on both sides"


def _close(got, ref, what):
    tol = 1e-5 * float(ref.abs().max())
    err = float((got.double() - ref).abs().max())
    assert err <= tol, (what, err, tol)
    assert bool((got[ref == 0] == 0).all()), (what, "gradients that are exactly 0 in the reference must be 0")


@pytest.mark.parametrize("mask", MASKS)
def test_mean_gradient_matches_autograd_of_the_oracle(mask):
    from causal_gen_amd import dmol
    from oracle import dmol_ref

    g = torch.Generator().manual_seed(11 + MASKS.index(mask))
    l, pre, s = _mean_logits(mask, g)
    _branches_hit(pre, s)
    gx = torch.randn(*l.shape[:-1], 3, generator=g)
    gs = torch.randn(*l.shape[:-1], 3, generator=g)

    l64 = l.double().requires_grad_(True)
    rx, rs = dmol_ref.dmol_mean(l64, mask)
    ((rx * gx.double()).sum() + (rs * gs.double()).sum()).backward()
    ref = l64.grad

    lc = l.cuda()
    with torch.no_grad():
        x0, s0 = dmol.mean_discretized_mix_logistic(lc, 10, mask, return_scale=True)
    grads = []
    for _ in range(2):
        lg = lc.clone().requires_grad_(True)
        x, sc = dmol.mean_discretized_mix_logistic(lg, 10, mask, return_scale=True)
        assert x.grad_fn is not None and sc.grad_fn is not None
        assert torch.equal(x, x0) and torch.equal(sc, s0)
        ((x * gx.cuda()).sum() + (sc * gs.cuda()).sum()).backward()
        grads.append(lg.grad.cpu())
    assert torch.equal(grads[0], grads[1]), "two backward runs must be bit-identical"
    got = grads[0]
    _close(got, ref, mask)
    if mask.startswith("top"):
        _, keep = _sel(l.double(), mask)
        assert (~keep).any()
        assert bool((got[..., :10][~keep] == 0).all()) and bool((ref[..., :10][~keep] == 0).all())
    if mask == "hard":
        assert bool((got[..., :10] == 0).all())
    # x alone (the scale output unused) takes the same path with no scale gradient
    lg = lc.clone().requires_grad_(True)
    (dmol.mean_discretized_mix_logistic(lg, 10, mask) * gx.cuda()).sum().backward()
    l64 = l.double().requires_grad_(True)
    (dmol_ref.dmol_mean(l64, mask)[0] * gx.double()).sum().backward()
    _close(lg.grad.cpu(), l64.grad, mask + " x only")


def _uniforms(seed, offset, n):
    gi = np.arange(n, dtype=np.uint64)
    r, r2, r3 = (_philox_words(seed, offset, 977, gi * np.uint64(4) + np.uint64(k)) for k in range(3))
    mixw = np.concatenate([r, r2, r3[:, :2]], 1)
    pixw = np.stack([r3[:, 2], r3[:, 3], r2[:, 3] ^ np.uint32(0x9E3779B9)], 1)
    f = lambda wds: torch.from_numpy(np.float32(1e-5) + np.float32(1.0 - 2e-5) * _u01(wds))
    return f(mixw), f(pixw)


@pytest.mark.parametrize("t", [None, 0.7])
def test_sample_gradient_matches_autograd_of_the_oracle_on_the_kernels_own_uniforms(t):
    from causal_gen_amd import dmol
    from oracle import dmol_ref

    B, H, W = 2, 8, 8
    g = torch.Generator().manual_seed(23 if t is None else 29)
    dev = torch.device("cuda", torch.cuda.current_device())
    with torch.no_grad():
        dmol.sample_from_discretized_mix_logistic(torch.zeros(1, 1, 1, 100, device=dev), 10)  # the free rng exists from here on
    rng = dmol._FREE_RNG[dev]
    start = rng.clone()
    seed, off = (int(v) for v in start.cpu())
    u_mix, u_pix = _uniforms(seed, off + 1, B * H * W)  # (each call advances the offset by one before it draws)
    u_mix, u_pix = u_mix.view(B, H, W, 10), u_pix.view(B, H, W, 3)
    l = _draw((B, H, W), g)
    for _ in range(50):
        l64 = l.double()
        v = (l64[..., :10] - torch.log(-torch.log(u_mix.double()))).sort(-1, descending=True)[0]
        sel = torch.nn.functional.one_hot((l64[..., :10] - torch.log(-torch.log(u_mix.double()))).argmax(-1), 10).double()
        nz = torch.log(u_pix.double()) - torch.log(1 - u_pix.double())
        pre, s = _chain(l64, sel, nz, t)
        bad = ((pre.abs() - 1).abs() < EDGE).any(-1) | ((s + 7).abs() < EDGE).any(-1) | ((v[..., 0] - v[..., 1]) < EDGE)
        if not bad.any():
            break
        l[bad] = _draw((int(bad.sum()),), g)
    assert not bad.any()
    _branches_hit(pre, s)
    gx = torch.randn(B, H, W, 3, generator=g)
    gs = torch.randn(B, H, W, 3, generator=g)

    l64 = l.double().requires_grad_(True)
    rx, rs = dmol_ref.dmol_sample(l64, t=t, u_mix=u_mix.double(), u_pix=u_pix.double())
    ((rx * gx.double()).sum() + (rs * gs.double()).sum()).backward()

    lg = l.cuda().requires_grad_(True)
    x, sc = dmol.sample_from_discretized_mix_logistic(lg, 10, return_scale=True, t=t)
    assert int(rng[1]) == off + 1
    assert float((x.detach().cpu().double() - rx.detach()).abs().max()) < 1e-4
    dmol.sample_from_discretized_mix_logistic(lg.detach(), 10)  # a later draw advances the free rng: backward must not see it
    ((x * gx.cuda()).sum() + (sc * gs.cuda()).sum()).backward()
    _close(lg.grad.cpu(), l64.grad, f"sample t={t}")


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("mask", ["soft", "hard", "top3"])
def test_fused_cf_step_matches_autograd_of_the_oracle(dtype, mask):
    from causal_gen_amd import dmol
    from oracle import dmol_ref

    B, H, W = 2, 8, 8
    eng, _ = make_engine([torch.nn.Conv2d(1, 1, 1)], [[1]], dtype)
    g = torch.Generator().manual_seed(41 + ["soft", "hard", "top3"].index(mask))
    mode = dmol._mask_mode(mask)
    # the logits as the engine stores them (binary16-rounded for f16) are what the oracle differentiates
    # log-scales around -1.5: the cf step's u = (x - rec_loc) / rec_scale stays O(1), so both sides of its clamp are hit
    rec = _mean_logits(mask, g, ls_mu=-1.5, dtype=eng.tdtype)[0].to(eng.tdtype)
    cf = _mean_logits(mask, g, ls_mu=-1.5, dtype=eng.tdtype)[0].to(eng.tdtype)
    x = ((torch.randint(0, 256, (B, H, W, 3), generator=g).float() - 127.5) / 127.5).to(eng.tdtype)
    gcf = torch.randn(B, 3, H, W, generator=g)
    gscale = 1.0 / 3.0

    r64, c64 = rec.double().requires_grad_(True), cf.double().requires_grad_(True)
    rl, rsc = dmol_ref.dmol_mean(r64, mask)
    cl, csc = dmol_ref.dmol_mean(c64, mask)
    u = (x.double() - rl) / rsc.clamp(min=1e-12)
    y = cl + csc * u
    cfx = torch.clamp(y, min=-1, max=1)
    (cfx * gcf.permute(0, 2, 3, 1).double()).sum().mul(gscale).backward()
    # a cf value NEAR a clamp end could take either branch in f32 (exactly on it -- x = rec_loc = +-1 and cf_loc = +-1 -- it is
    # exact in both precisions)
    d = (y.detach().abs() - 1).abs()
    assert not bool(((d > 0) & (d < 1e-4)).any())
    assert bool((y.detach().abs() < 1).any()) and bool((y.detach().abs() > 1).any())

    rt, ct, xt = (eng.wrap_nhwc(v.cuda().contiguous()) for v in (rec, cf, x))
    g_rec, g_cf = eng.new(B, H, W, 100), eng.new(B, H, W, 100)
    gd = gcf.cuda().contiguous()
    eng.lib.cf_dmol_bwd(eng.dt, B, H, W, mode, rt.cv(), ct.cv(), xt.cv(), gd.data_ptr(), gscale, g_rec.cv(), g_cf.cv(), eng.stream)
    torch.cuda.synchronize()
    tol = 1e-5 if dtype == "f32" else 2e-3
    for got_t, ref, what in ((g_rec, r64.grad, "rec"), (g_cf, c64.grad, "cf")):
        got = eng.to_nchw(got_t).permute(0, 2, 3, 1).cpu().double()
        err = float((got - ref).abs().max())
        assert err <= tol * float(ref.abs().max()), (what, err, float(ref.abs().max()))
        assert bool((got[ref == 0] == 0).all()), what


def _dmol_model(name="tiny_dmol_c3.pt"):
    from causal_gen_amd import dmol, vae
    from causal_gen_amd.hps import Hparams

    fx = load_golden(name)
    hpd = dict(fx["hp"])
    args = Hparams(**hpd)
    m = vae.HVAE(args)
    m.likelihood = dmol.DmolNet(args)
    m.load_state_dict(fx["state_dict"])
    m.compute_dtype = "f32"
    return fx, hpd, m.cuda().eval()


@pytest.mark.parametrize("particles", [1, 2])
def test_dscm_forward_with_a_dmol_head_matches_oracle_values_and_gradients(particles):
    fx, hpd, m = _dmol_model()
    _dscm_case(fx, hpd, m, "tiny_dmol_c3", particles)


def test_dscm_forward_with_a_dmol_head_at_cmnist_size():
    """BASELINE config 3's model: the cmnist HVAE with DmolNet swapped in (exogenous prior), perturbed weights, two particles,
    against oracle/dscm_ref.py run live on the CPU."""
    from causal_gen_amd import dmol, vae
    from causal_gen_amd.hps import setup_hparams
    from oracle import fullsize_recipe as R

    hp = setup_hparams("cmnist", cond_prior=False)
    torch.manual_seed(7)
    m = vae.HVAE(hp)
    dmol.use_dmol(m, hp)
    m.apply(R.init_bias)
    R.perturb(m)
    x, pa = R.inputs(hp, 2)
    fx = {"x": x, "pa": pa, "cf_pa": pa.roll(1, 0) * 0.5, "state_dict": {k: v.detach().clone() for k, v in m.state_dict().items()}}
    m.compute_dtype = "f32"
    _dscm_case(fx, dict(vars(hp)), m.cuda().eval(), "cmnist+dmol", 2)


def test_cf_branch_alone_reaches_the_weights_through_the_dmol_head():
    from causal_gen_amd import vae as hvae_mod
    from oracle import dscm_ref, hvae_ref

    fx, hpd, m = _dmol_model()
    hp = SimpleNamespace(**hpd)
    x, pa, cf = fx["x"], fx["pa"], fx["cf_pa"]
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in fx["state_dict"].items()}
    noise = hvae_ref._Noise(None)
    torch.manual_seed(3)
    ref = dscm_ref.dscm_forward(sd, hp, x, pa, [cf], 1.0, noise=noise)
    (ref["cf_x"] ** 2).sum().backward()
    m.noise = [e.clone() for e in noise.drawn]
    for p in m.parameters():
        p.requires_grad_(True)
    trig = torch.zeros(1, device="cuda", requires_grad=True)
    elbo, nll, kl, cf_x, _ = hvae_mod._DSCMFunction.apply(trig, m, x.cuda(), pa.cuda(), (cf.cuda(),), 1.0, 1.0)
    assert float((cf_x.detach().cpu() - ref["cf_x"].detach()).abs().max()) < 1e-3
    (cf_x ** 2).sum().backward()
    torch.cuda.synchronize()
    params = dict(m.named_parameters())
    for n_ in ("encoder.stem.weight", "decoder.blocks.0.posterior.conv.1.weight", "decoder.blocks.1.z_proj.weight",
               "likelihood.conv.weight"):
        rg = sd[n_].grad
        got = params[n_].grad.cpu()
        assert float(rg.abs().max()) > 0, n_
        assert float((got - rg).abs().max()) < 2e-3 * float(rg.abs().max()), n_
