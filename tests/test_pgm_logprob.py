"""The host density of the parent SCMs (causal_gen_amd.pgm: ``log_prob`` / ``nll``) in f64 on the CPU.  Every non-spline term is
held to the ``torch.distributions`` construction of the same thing; the spline's log-Jacobian to autograd through the existing
``LinearSpline.forward``, its density to integrating to one, and to the plain normal density outside the bound.  Bound 1e-9
throughout: f64 against f64, only the order of operations differs."""
import math

import pytest
import torch
import torch.distributions as D
from torch.distributions.transforms import AffineTransform, SigmoidTransform

import pgm_cases as PC

TOL = 1e-9


def _case(kind, n=33, **kw):
    m = PC.to64(PC.make_pgm(kind, **kw))
    obs = PC.cast(PC.draw(m.float(), n), torch.float64)
    return m.double(), obs


def _close(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a - b).abs().max().item()
    assert err <= TOL, err


@pytest.mark.parametrize("kind,var,logit", [("flow", "sex", "s_logit"), ("flow", "mri_seq", "m_logit"), ("chest", "sex", "sex_logit")])
def test_bernoulli_roots(kind, var, logit):
    m, obs = _case(kind)
    with torch.no_grad():
        want = D.Bernoulli(logits=getattr(m, logit)).log_prob(obs[var]).sum(-1)
        _close(m.log_prob(obs)[var], want)


@pytest.mark.parametrize("kind,var,logits", [("morpho", "digit", "digit_logits"), ("colour", "digit", "digit_logits"),
                                             ("colour", "colour", "colour_logits"), ("chest", "race", "race_logits")])
def test_categorical_roots(kind, var, logits):
    m, obs = _case(kind)
    with torch.no_grad():
        want = D.OneHotCategorical(logits=getattr(m, logits)).log_prob(obs[var])
        _close(m.log_prob(obs)[var], want)


@pytest.mark.parametrize("widths", ([32, 32], [8, 16], [64], [64, 64, 64]))
def test_conditional_affine_terms(widths):
    m, obs = _case("flow", widths=widths)
    with torch.no_grad():
        lp = m.log_prob(obs)
        for var, flow, ctx in (("brain_volume", m.bvol_flow, ("sex", "age")), ("ventricle_volume", m.vvol_flow, ("brain_volume", "age"))):
            loc, ls = flow.params(torch.cat([obs[c] for c in ctx], 1))
            dist = D.TransformedDistribution(D.Normal(torch.zeros_like(loc), torch.ones_like(loc)), [AffineTransform(loc, ls.exp())])
            _close(lp[var], dist.log_prob(obs[var]).sum(-1))
    m, obs = _case("morpho", widths=widths)
    with torch.no_grad():
        loc, ls = m.context_nn.params(obs["thickness"])
        dist = D.TransformedDistribution(D.Normal(torch.zeros_like(loc), torch.ones_like(loc)),
                                         [AffineTransform(loc, ls.exp()), SigmoidTransform(), AffineTransform(-1.0, 2.0)])
        _close(m.log_prob(obs)["intensity"], dist.log_prob(obs["intensity"]).sum(-1))


def test_gumbel_max_finding_is_the_categorical_log_prob():
    m, obs = _case("chest", n=64)
    assert 0 < obs["finding"].sum() < 64  # (both classes occur)
    with torch.no_grad():
        want = D.Categorical(logits=m.finding_logits(obs["age"])).log_prob(obs["finding"].squeeze(-1))
        _close(m.log_prob(obs)["finding"], want)


@pytest.mark.parametrize("bins", (4, 8))
def test_spline_log_jacobian_is_autograd_of_forward(bins):
    from causal_gen_amd.pgm import LinearSpline

    torch.manual_seed(bins)
    sp = LinearSpline(1, count_bins=bins).double()
    eps = torch.cat([torch.linspace(-3.5, 3.5, 211, dtype=torch.float64), torch.tensor([-3.0, 3.0], dtype=torch.float64)])[:, None]
    eps.requires_grad_(True)
    y = sp(eps)
    dy, = torch.autograd.grad(y.sum(), eps)
    with torch.no_grad():
        x, log_det = sp.inv_and_log_det(y.detach())
        _close(x, eps.detach())
        _close(log_det, dy.log())
        _close(x, sp.inv(y.detach()))
        outside = (eps.detach().abs() >= 3.0).squeeze(-1)
        assert outside.sum() >= 2 and bool((log_det[outside] == 0).all())


@pytest.mark.parametrize("kind,var,bins", [("flow", "age", 4), ("chest", "age", 8)])
def test_spline_density_integrates_to_one_and_is_normal_outside_the_bound(kind, var, bins):
    m, obs = _case(kind, n=2)
    sp = PC.spline_of(m)
    assert sp.count_bins == bins
    n = 2_000_001
    u = torch.linspace(-8.0, 8.0, n, dtype=torch.float64)[:, None]
    with torch.no_grad():
        eps, log_det = sp.inv_and_log_det(u)
        dens = torch.exp(-0.5 * eps * eps - 0.5 * math.log(2 * math.pi) - log_det).squeeze(-1)
        total = torch.trapezoid(dens, dx=16.0 / (n - 1)).item()
        assert abs(total - 1.0) <= TOL, total
        # through log_prob itself, rows outside the bound: the plain normal density
        out = torch.tensor([[-3.0], [3.0], [3.25], [-7.5]], dtype=torch.float64)
        o = {k: v[:1].expand(len(out), -1).clone() for k, v in obs.items()}
        o[var] = out
        _close(m.log_prob(o)[var], D.Normal(0.0, 1.0).log_prob(out).sum(-1))
        # and one inside, against the integrand above
        o[var] = u[n // 3:n // 3 + 4]
        _close(m.log_prob(o)[var].exp(), dens[n // 3:n // 3 + 4])


def test_normalised_spline_term_of_morpho_thickness():
    from causal_gen_amd.pgm import normalize_inv

    m, obs = _case("morpho")
    with torch.no_grad():
        u = normalize_inv(obs["thickness"])
        eps, log_det = m.thickness_module[0].inv_and_log_det(u)
        # density of x = 2 sigmoid(u) - 1: the Jacobian of the normalisation through torch's own transforms
        norm = AffineTransform(-1.0, 2.0).log_abs_det_jacobian(torch.sigmoid(u), None) + SigmoidTransform().log_abs_det_jacobian(u, None)
        want = (D.Normal(0.0, 1.0).log_prob(eps) - log_det - norm).sum(-1)
        _close(m.log_prob(obs)["thickness"], want)


@pytest.mark.parametrize("kind", PC.KINDS)
def test_nll_is_the_sum_of_the_terms_over_the_batch(kind):
    m, obs = _case(kind, n=17)
    with torch.no_grad():
        lp = m.log_prob(obs)
        assert set(lp) == set(m.variables) and all(v.shape == (17,) for v in lp.values())
        want = -torch.stack([v for v in lp.values()]).sum() / 17
        assert abs(m.nll(obs).item() - want.item()) <= TOL
    loss = m.nll(obs)
    loss.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())


@pytest.mark.parametrize("kind", PC.KINDS)
def test_log_prob_leaves_counterfactual_untouched(kind):
    m, obs = _case(kind, n=9)
    var = next(iter(m.variables))
    do = {var: obs[var].flip(0)}
    if kind == "chest":
        m.generator = torch.Generator().manual_seed(5)
    before = m.counterfactual(obs, do)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m.nll(obs).backward()
    if kind == "chest":
        m.generator = torch.Generator().manual_seed(5)
    after = m.counterfactual(obs, do)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
