"""DSCM.forward with the real anticausal predictor as elbo_fn (``AnticausalELBO``) under autograd: aux_loss, loss, the
multiplier's gradient and every HVAE weight gradient against oracle/dscm_ref.dscm_forward with aux_fn = the f64 predictor loss / B
(tests/predictor_ref.py), on the tiny DGauss / DMoL fixtures and at morphomnist / cmnist size.  The predictor's input gradient
reaches the HVAE through cf_x, which comes off the engine tape of the counterfactual passes."""
from types import SimpleNamespace

import pytest
import torch

from conftest import load_golden
from predictor_ref import predictor_nll, randomise
from test_gpu_dscm import StubPGM

pytestmark = pytest.mark.gpu


def _predictor(kind, C, R, seed=11):
    from causal_gen_amd import predictor as P

    pred = P.make_predictor(SimpleNamespace(dataset=kind, input_channels=C, input_res=R, std_fixed=0.0))
    randomise(pred, torch.Generator().manual_seed(seed))
    with torch.no_grad():  # strong classifier heads: the aux gradient is not small next to the ELBO's
        for name in ("encoder_y", "encoder_c"):
            if hasattr(pred, name):
                getattr(pred, name).fc[3].weight.mul_(4.0)
    return pred.cuda()


def _pred_obs(kind, B, g):
    oh = lambda: torch.nn.functional.one_hot(torch.randint(0, 10, (B,), generator=g), 10).float()
    if kind == "morphomnist":
        return {"thickness": torch.rand(B, 1, generator=g) * 1.6 - 0.8, "intensity": torch.rand(B, 1, generator=g) * 1.6 - 0.8,
                "digit": oh()}
    return {"digit": oh(), "colour": oh()}


def _case(fx, hpd, m, kind, particles, name):
    from causal_gen_amd import dscm
    from causal_gen_amd.predictor import AnticausalELBO
    from oracle import dscm_ref, hvae_ref

    hp = SimpleNamespace(**hpd)
    x, pa, cf = fx["x"], fx["pa"], fx["cf_pa"]
    B, ctx, C, R = x.shape[0], pa.shape[1], x.shape[1], x.shape[-1]
    names = [f"p{i}" for i in range(ctx)]
    beta, t_ab, lmbda0, eps_c, damping = 1.7, 0.9, 0.8, 2.0, 10.0
    g = torch.Generator().manual_seed(5)
    pobs = _pred_obs(kind, B, g)
    # the counterfactual values of the predictor's variables (what pgm.counterfactual returns for the last particle)
    pcf = {k: (v.roll(1, 0) if v.shape[1] > 1 else -0.5 * v) for k, v in pobs.items()}
    pred = _predictor(kind, C, R)

    # ---- oracle
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in fx["state_dict"].items()}
    lm = torch.tensor([lmbda0], requires_grad=True)
    noise = hvae_ref._Noise(None)
    torch.manual_seed(17)
    cf_list = [torch.cat([cf[:, :1] * (1.0 + 0.5 * p), pa[:, 1:]], 1) for p in range(particles)]
    aux_fn = lambda c: (predictor_nll(pred, dict(pcf, x=c.double())) / B).float()
    ref = dscm_ref.dscm_forward(sd, hp, x, pa, cf_list, beta, t_abduct=t_ab, noise=noise, aux_fn=aux_fn, lmbda=lm,
                                eps=torch.tensor([eps_c]), damping=damping)
    ref["loss"].sum().backward()

    # ---- HIP path through DSCM with the real predictor and AnticausalELBO
    class SeqPGM(StubPGM):
        def __init__(self):
            super().__init__()
            self.i = 0

        def counterfactual(self, obs, intervention, num_particles=1):
            out = dict(obs)
            out["p0"] = cf[:, 0, 0, 0].cuda() * (1.0 + 0.5 * self.i)
            out.update({k: v.cuda() for k, v in pcf.items()})
            self.i += 1
            return out

    args = SimpleNamespace(**{**hpd, "parents_x": names, "dataset": "none", "lmbda_init": lmbda0, "elbo_constraint": eps_c, "damping": damping})
    args.beta = beta
    model = dscm.DSCM(args, SeqPGM(), pred, m).cuda()
    for p in m.parameters():
        p.requires_grad_(True)
    obs = {"x": x.cuda()}
    obs.update({n: pa[:, i, 0, 0].cuda() for i, n in enumerate(names)})
    obs.update({k: v.cuda() for k, v in pobs.items()})
    m.noise = [e.clone() for e in noise.drawn]
    out = model(obs, {"p0": None}, AnticausalELBO(), cf_particles=particles, t_abduct=t_ab)
    assert not m.noise
    got_aux, want_aux = float(out["aux_loss"].detach()), float(ref["aux_loss"].detach())
    assert abs(got_aux - want_aux) <= 2e-4 * abs(want_aux) + 1e-5, (got_aux, want_aux)
    assert abs(float(out["loss"].detach()) - float(ref["loss"].detach())) <= 2e-4 * abs(float(ref["loss"].detach())) + 1e-5
    out["loss"].sum().backward()
    torch.cuda.synchronize()
    assert abs(float(model.lmbda.grad) - float(lm.grad)) <= 1e-4 * abs(float(lm.grad)) + 1e-6
    assert all(p.grad is None for p in pred.parameters()), "the predictor is frozen"
    n_checked = 0
    for n_, p in m.named_parameters():
        rg = sd[n_].grad
        if rg is None or float(rg.abs().max()) == 0.0:
            continue
        assert p.grad is not None, n_
        d = float((p.grad.cpu() - rg).abs().max()) / float(rg.abs().max())
        l2 = float((p.grad.cpu() - rg).norm()) / float(rg.norm())
        assert d < 5e-3 and l2 < 2e-3, (name, n_, d, l2)
        n_checked += 1
    assert n_checked > 20


def _aux_only(fx, hpd, m, kind):
    """loss = aux_loss alone: the HVAE weight gradient is the predictor's input gradient carried back through cf_x."""
    from causal_gen_amd import vae as hvae_mod
    from causal_gen_amd.predictor import AnticausalELBO
    from oracle import dscm_ref, hvae_ref

    hp = SimpleNamespace(**hpd)
    x, pa, cf = fx["x"], fx["pa"], fx["cf_pa"]
    B, C, R = x.shape[0], x.shape[1], x.shape[-1]
    pobs = _pred_obs(kind, B, torch.Generator().manual_seed(9))
    pred = _predictor(kind, C, R, seed=13)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in fx["state_dict"].items()}
    noise = hvae_ref._Noise(None)
    torch.manual_seed(3)
    ref = dscm_ref.dscm_forward(sd, hp, x, pa, [cf], 1.0, noise=noise)
    (predictor_nll(pred, dict(pobs, x=ref["cf_x"].double())) / B).backward()
    m.noise = [e.clone() for e in noise.drawn]
    for p in m.parameters():
        p.requires_grad_(True)
    trig = torch.zeros(1, device="cuda", requires_grad=True)
    _, _, _, cf_x, _ = hvae_mod._DSCMFunction.apply(trig, m, x.cuda(), pa.cuda(), (cf.cuda(),), 1.0, 1.0)
    aux = AnticausalELBO().differentiable_loss(pred.model_anticausal, pred.guide_pass,
                                               **dict({k: v.cuda() for k, v in pobs.items()}, x=cf_x)) / B
    aux.backward()
    torch.cuda.synchronize()
    params = dict(m.named_parameters())
    checked = 0
    for n_, p in params.items():
        rg = sd[n_].grad
        if rg is None or float(rg.abs().max()) == 0.0:
            continue
        got = p.grad.cpu()
        assert float((got - rg).abs().max()) < 2e-3 * float(rg.abs().max()), n_
        checked += 1
    assert checked > 20


def _build(name):
    from causal_gen_amd import dmol, vae
    from causal_gen_amd.hps import Hparams

    fx = load_golden(name)
    hpd = dict(fx["hp"])
    args = Hparams(**hpd)
    m = vae.HVAE(args)
    if "dmol" in name:
        m.likelihood = dmol.DmolNet(args)
    m.load_state_dict(fx["state_dict"])
    m.compute_dtype = "f32"
    return fx, hpd, m.cuda().eval()


@pytest.mark.parametrize("name,kind,particles", [("tiny_default_c1.pt", "morphomnist", 1), ("tiny_default_c1.pt", "morphomnist", 2),
                                                 ("tiny_dmol_c3.pt", "cmnist", 1)])
def test_dscm_with_anticausal_elbo_on_tiny_fixtures(name, kind, particles):
    fx, hpd, m = _build(name)
    _case(fx, hpd, m, kind, particles, name)


@pytest.mark.parametrize("name,kind", [("tiny_default_c1.pt", "morphomnist"), ("tiny_dmol_c3.pt", "cmnist")])
def test_aux_loss_alone_reaches_the_hvae_weights(name, kind):
    fx, hpd, m = _build(name)
    _aux_only(fx, hpd, m, kind)


@pytest.mark.parametrize("kind", ["morphomnist", "cmnist"])
def test_dscm_with_anticausal_elbo_at_preset_size(kind):
    from causal_gen_amd import dmol, vae
    from causal_gen_amd.hps import setup_hparams
    from oracle import fullsize_recipe as R

    hp = setup_hparams(kind, cond_prior=False)
    torch.manual_seed(7)
    m = vae.HVAE(hp)
    if kind == "cmnist":
        dmol.use_dmol(m, hp)
    m.apply(R.init_bias)
    R.perturb(m)
    x, pa = R.inputs(hp, 2)
    fx = {"x": x, "pa": pa, "cf_pa": pa.roll(1, 0) * 0.5, "state_dict": {k: v.detach().clone() for k, v in m.state_dict().items()}}
    m.compute_dtype = "f32"
    _case(fx, dict(vars(hp)), m.cuda().eval(), kind, 2, kind)
