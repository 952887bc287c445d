"""``cf_train.CfTrainStep`` on the tiny DGauss / DMoL fixtures with the real anticausal predictors (the pairs of
tests/test_gpu_predictor_dscm.py): gradients against oracle/dscm_ref and against ``DSCM.forward(...).backward()`` on the device, a
three-step trajectory against the oracle with a constant lr, graph replay against eager execution, the skip and NaN paths,
``step_from`` against ``step()``, the intervention's mask word, the checkpoint round trip and the weight images after a step.

Device step against ``DSCM.forward(...).backward()`` (same kernels, same noise; the seeds w S / (B dims) are rounded on the device in
f32 where the host composition rounds torch's 0-dim arithmetic): measured worst deviation relative to a parameter gradient's
largest element 0.0 on both fixtures (bit-equal; LABNOTES 36), so the bound is 0: equality.

Multiplier against the oracle in the trajectory: Adam's update m^ / sqrt(v^) is homogeneous of degree 0 in the gradient history and
at most sqrt(1 / (1 - b2)) ~ 3.2 in size; a relative error delta in each gradient g = eps - elbo (|d elbo| <= 2e-4 |elbo| + 1e-5, the
values' bound) moves it by at most 2 delta 3.2, so after k steps |d lmbda| <= k lr_lagrange 6.4 delta (+ 1e-6 for f32 rounding)."""
import copy
from types import SimpleNamespace

import pytest
import torch

import cf_train_ref as R
import pgm_cases as PC
from predictor_ref import predictor_nll
from test_gpu_dscm import StubPGM
from test_gpu_predictor_dscm import _build, _pred_obs, _predictor

pytestmark = pytest.mark.gpu

BETA, T_AB, LMBDA0, EPS_C, DAMPING = 1.7, 0.9, 0.8, 2.0, 10.0
LR, LR_LAG = 1e-3, 1e-2
HOST_BOUND = 0.0  # device step against DSCM.forward.backward: min(4 x the measured deviation, 1e-5), see the docstring
GRAD_SKIP = 1e5   # w = lmbda - damping (eps - elbo) is ~58 on these fixtures: the fixtures' own threshold of 500 would drop most steps
PAIRS = [("tiny_default_c1.pt", "morphomnist"), ("tiny_dmol_c3.pt", "cmnist")]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


class _FixedPGM(StubPGM):
    """``pgm.counterfactual`` of the host composition: the observed parents with p0 and the predictor's variables replaced."""

    def __init__(self, cf_p0, pcf):
        super().__init__()
        self.cf_p0, self.pcf = cf_p0, pcf

    def counterfactual(self, obs, intervention, num_particles=1):
        out = dict(obs)
        out["p0"] = self.cf_p0.cuda()
        out.update({k: v.cuda() for k, v in self.pcf.items()})
        return out


def _make(name, kind, use_graph=False, ema=True, **over):
    """(fixture, hyper-parameters, DSCM on the device, CfTrainStep, the predictor's factual and counterfactual variables)"""
    from causal_gen_amd import dscm
    from causal_gen_amd.cf_train import CfTrainStep

    fx, hpd, m = _build(name)
    # (DSCM.forward's counterfactual parents: p0 under the intervention, the others as observed)
    fx["cf_pa"] = torch.cat([fx["cf_pa"][:, :1], fx["pa"][:, 1:]], 1)
    x, pa, cf = fx["x"], fx["pa"], fx["cf_pa"]
    B, ctx, C, R_ = x.shape[0], pa.shape[1], x.shape[1], x.shape[-1]
    pobs = _pred_obs(kind, B, torch.Generator().manual_seed(5))
    pcf = {k: (v.roll(1, 0) if v.shape[1] > 1 else -0.5 * v) for k, v in pobs.items()}
    pred = _predictor(kind, C, R_)
    args = SimpleNamespace(**{**hpd, "parents_x": [f"p{i}" for i in range(ctx)], "dataset": "none", "lmbda_init": LMBDA0,
                              "elbo_constraint": EPS_C, "damping": DAMPING, "beta": BETA, "grad_skip": GRAD_SKIP, **over})
    model = dscm.DSCM(args, _FixedPGM(cf[:, 0, 0, 0], pcf), pred, m).cuda()
    for p in m.parameters():
        p.requires_grad_(True)
    step = CfTrainStep(model, args, lr=LR, lr_lagrange=LR_LAG, ema=ema, use_graph=use_graph)
    step.t_abduct = T_AB
    return fx, hpd, model, step, pobs, pcf


def _oracle(sd, hpd, fx, pred, pcf, lm, noise):
    from oracle import dscm_ref

    x, pa, cf = fx["x"], fx["pa"], fx["cf_pa"]
    B = x.shape[0]
    aux_fn = lambda c: (predictor_nll(pred, dict(pcf, x=c.double())) / B).float()  # noqa: E731
    return dscm_ref.dscm_forward(sd, SimpleNamespace(**hpd), x, pa, [cf], BETA, t_abduct=T_AB, noise=noise, aux_fn=aux_fn, lmbda=lm,
                                 eps=torch.tensor([EPS_C]), damping=DAMPING)


def _close(got, want, rel=2e-4, ab=1e-5):
    return abs(float(got) - float(want)) <= rel * abs(float(want)) + ab


@pytest.mark.parametrize("name,kind", PAIRS)
def test_loss_and_grads_match_the_oracle_and_the_host_composition(name, kind):
    from causal_gen_amd.predictor import AnticausalELBO
    from oracle import hvae_ref

    fx, hpd, model, step, pobs, pcf = _make(name, kind)
    m, x, pa, cf = model.vae, fx["x"], fx["pa"], fx["cf_pa"]
    names = model.args.parents_x
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in fx["state_dict"].items()}
    lm = torch.tensor([LMBDA0], requires_grad=True)
    noise = hvae_ref._Noise(None)
    torch.manual_seed(17)
    ref = _oracle(sd, hpd, fx, model.predictor, pcf, lm, noise)
    ref["loss"].sum().backward()

    # the host composition on the device: DSCM.forward under autograd, same noise
    obs = {"x": x.cuda()}
    obs.update({n: pa[:, i, 0, 0].cuda() for i, n in enumerate(names)})
    obs.update({k: v.cuda() for k, v in pobs.items()})
    m.noise = [e.clone() for e in noise.drawn]
    out = model(obs, {"p0": None}, AnticausalELBO(), cf_particles=1, t_abduct=T_AB)
    out["loss"].sum().backward()
    torch.cuda.synchronize()
    host = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    host_lm, host_loss = float(model.lmbda.grad), float(out["loss"].detach())

    m.noise = [e.clone() for e in noise.drawn]
    loss, aux, out3, g_l, grads = step.loss_and_grads(x.cuda(), pa.cuda(), cf.cuda(), pcf)
    torch.cuda.synchronize()
    assert not m.noise
    for got, key in ((loss, "loss"), (aux, "aux_loss"), (out3[0], "elbo"), (out3[1], "nll"), (out3[2], "kl")):
        assert _close(got, ref[key].detach().reshape(-1)[0]), (key, float(got), float(ref[key].detach().reshape(-1)[0]))
    assert abs(float(g_l) - float(lm.grad)) <= 1e-4 * abs(float(lm.grad)) + 1e-6
    checked, worst = 0, 0.0
    for n_, p in m.named_parameters():
        rg = sd[n_].grad
        if rg is None or float(rg.abs().max()) == 0.0:
            continue
        g = grads[n_].cpu()
        d = float((g - rg).abs().max()) / float(rg.abs().max())
        l2 = float((g - rg).norm()) / float(rg.norm())
        assert d < 5e-3 and l2 < 2e-3, (name, n_, d, l2)
        worst = max(worst, float((grads[n_] - host[n_]).abs().max()) / float(host[n_].abs().max()))
        checked += 1
    assert checked > 20
    print(f"{name}: device step against DSCM.forward.backward: worst relative-to-max deviation {worst:.3e}, "
          f"loss {float(loss)!r} against {host_loss!r}, g_lmbda {float(g_l)!r} against {host_lm!r}")
    assert worst <= HOST_BOUND
    assert _close(loss, host_loss, 1e-6, 1e-7) and _close(g_l, host_lm, 1e-6, 1e-7)
    assert step.epoch_stats()["n"] == 0  # loss_and_grads leaves the running sums alone


def _adamw64(p, g, m, v, c, t0, lr, b1, b2, wd):
    gc = g * c
    m = m + (gc - m) * (1 - b1)
    v = v * b2 + (1 - b2) * gc * gc
    t = t0 + 1
    denom = v.sqrt() / (1 - b2 ** t) ** 0.5 + 1e-8
    return p * (1 - lr * wd) - lr / (1 - b1 ** t) * m / denom, m, v


@pytest.mark.parametrize("name,kind", PAIRS)
def test_three_steps_match_the_oracle_trajectory(name, kind):
    from oracle import hvae_ref, train_ref

    fx, hpd, model, step, pobs, pcf = _make(name, kind)
    m, x, pa, cf = model.vae, fx["x"], fx["pa"], fx["cf_pa"]
    hp = SimpleNamespace(**{**hpd, "lr": LR, "grad_skip": GRAD_SKIP})
    tr = train_ref.RefTrainer(dict(fx["state_dict"], lmbda=torch.tensor([LMBDA0])), hp)
    tr.warm = lambda it: 1.0  # train_cf.py has no scheduler: a constant lr
    lag = [LMBDA0, 0.0, 0.0, LMBDA0]  # the oracle's multiplier, its moments and EMA (f64)
    eng = step.eng
    p64, e64 = eng.flat_p.double().clone(), step.ema_flat.double().clone()
    m64, v64 = torch.zeros_like(p64), torch.zeros_like(p64)
    b1, b2 = hpd["betas"]
    tol_lm = 1e-6
    for it in range(3):
        noise = hvae_ref._Noise(None)
        torch.manual_seed(100 + it)
        sd = {k: v for k, v in tr.sd.items() if k != "lmbda"}
        lm = tr.sd["lmbda"]
        ref = _oracle(sd, hpd, fx, model.predictor, pcf, lm, noise)
        keys = [k for k in tr.sd]
        gs = torch.autograd.grad(ref["loss"].sum(), [tr.sd[k] for k in keys], allow_unused=True)
        grads = dict(zip(keys, gs))
        want = {k: float(ref[k].detach().reshape(-1)[0]) for k in ("loss", "aux_loss", "elbo", "nll", "kl")}
        g_l = float(grads["lmbda"])
        t0 = tr.opt_steps
        total = tr.apply_grads(grads)
        assert tr.opt_steps == t0 + 1
        new = R.lagrange_step(*lag, g_l, train_ref.clip_coef(total, hp.grad_clip), t0, LR_LAG, (b1, b2), 1e-8, hp.ema_rate, 100)
        lag = [new[k][0] for k in ("lmbda", "m", "v", "ema")]
        with torch.no_grad():
            tr.sd["lmbda"].fill_(lag[0])  # (RefTrainer descended on it with the parameters' AdamW: its own optimiser decides)
        delta = (2e-4 * abs(want["elbo"]) + 1e-5) / abs(EPS_C - want["elbo"])
        tol_lm += LR_LAG * 6.4 * delta

        m.noise = [e.clone() for e in noise.drawn]
        out = step.step(x.cuda(), pa.cuda(), cf.cuda(), pcf)
        torch.cuda.synchronize()
        assert not m.noise
        st = step.stats()
        for k in want:
            print(it, k, float(out[k]), want[k])
            assert _close(out[k], want[k]), (it, k, float(out[k]), want[k])
        assert abs(st["grad_norm"] - total) / total < 2e-3, (it, st, total)
        assert st["opt_steps"] == tr.opt_steps and not st["skipped_last"]
        print(it, "lmbda", st["lmbda"], lag[0], tol_lm)
        assert abs(st["lmbda"] - lag[0]) <= tol_lm, (it, st["lmbda"], lag[0], tol_lm)
        # f64 AdamW fed the device's own gradient and clip coefficient
        g64 = eng.flat_g.double()
        for lo, hi in step.ranges:
            p64[lo:hi], m64[lo:hi], v64[lo:hi] = _adamw64(p64[lo:hi], g64[lo:hi], m64[lo:hi], v64[lo:hi], st["clip_coef"], t0, LR, b1, b2,
                                                          hpd["wd"])
            e64[lo:hi] = p64[lo:hi]  # (the EMA's copy phase: fewer than 100 steps)
    torch.testing.assert_close(eng.flat_p.double(), p64, rtol=2e-3, atol=2e-5)
    torch.testing.assert_close(step.ema_flat.double(), e64, rtol=2e-3, atol=2e-5)
    assert float(step.ema_model.lmbda.detach()) == float(model.lmbda.detach()) == step.stats()["lmbda"]
    es = step.epoch_stats()
    assert es["n"] == 3 and es["n_bad"] == 0 and step.epoch_stats()["n"] == 0


def _snapshot(model, step):
    torch.cuda.synchronize()
    return {"w": {k: v.clone() for k, v in model.vae.state_dict().items()}, "ema": {k: v.clone() for k, v in step.ema_vae.state_dict().items()},
            "lag": step.lag.clone(), "m": step.tail.m.clone(), "v": step.tail.v.clone(), "res": step.res.clone()}


def _trace(step, out):
    """Device-side copies (no host sync) of what a step computed: its values, its flat gradient, the tail's state (norm, clip)."""
    return {"out3": out["out3"].clone(), "res": step.res.clone(), "flat_g": step.eng.flat_g.clone(), "state": step.state.clone()}


def _same(a, b):
    for k in ("lag", "m", "v", "res"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    for part in ("w", "ema"):
        for k in a[part]:
            assert torch.equal(a[part][k], b[part][k]), (part, k)


@pytest.mark.parametrize("name,kind", PAIRS)
def test_graph_replay_equals_eager(name, kind):
    outs = []
    for use_graph in (False, True):
        torch.manual_seed(123)
        fx, hpd, model, step, pobs, pcf = _make(name, kind, use_graph=use_graph)
        first = None
        for _ in range(4):
            out = step.step(fx["x"].cuda(), fx["pa"].cuda(), fx["cf_pa"].cuda(), pcf)
            if first is None:  # (the call that captures returns this step's values, not the graph's unwritten output)
                first = torch.stack([out["elbo"], out["nll"], out["kl"], out["loss"], out["aux_loss"]]).clone(), out["out3"].clone()
        snap = _snapshot(model, step)
        outs.append((out["out3"].clone(), snap, step.stats(), step.graph_count(), first))
    (o0, s0, t0, g0, f0), (o1, s1, t1, g1, f1) = outs
    assert t0["opt_steps"] == t1["opt_steps"] == 4 and (g0, g1) == (0, 1)
    assert torch.equal(_bits(f0[0]), _bits(f1[0])) and torch.equal(_bits(f0[1]), _bits(f1[1])), (f0, f1)
    assert bool(torch.isfinite(f1[1]).all()) and torch.equal(_bits(f1[0][:3]), _bits(f1[1]))
    assert torch.equal(_bits(o0), _bits(o1)), (o0, o1)
    _same(s0, s1)
    assert t0["lmbda"] == t1["lmbda"] != LMBDA0


def test_skip_on_huge_gradient_leaves_everything_untouched():
    name, kind = PAIRS[0]
    fx, hpd, model, step, pobs, pcf = _make(name, kind, grad_skip=1e-6)  # every step is "too large"
    before = _snapshot(model, step)
    for _ in range(2):
        step.step(fx["x"].cuda(), fx["pa"].cuda(), fx["cf_pa"].cuda(), pcf)
    st = step.stats()
    assert st["n_skipped"] == 2 and st["opt_steps"] == 0 and st["skipped_last"] and st["n_bad"] == 0
    after = _snapshot(model, step)
    after["res"] = before["res"]  # (the step's own results are written; everything an optimiser owns is not)
    _same(before, after)
    assert step.epoch_stats()["n"] == 2  # the reference counts a step dropped for its norm in its statistics (train_cf.py:205)


def test_nan_in_x_drops_the_step():
    name, kind = PAIRS[0]
    fx, hpd, model, step, pobs, pcf = _make(name, kind)
    x = fx["x"].cuda()
    step.step(x, fx["pa"].cuda(), fx["cf_pa"].cuda(), pcf)
    before, sums = _snapshot(model, step), step.sums.clone()
    bad = x.clone()
    bad[1, 0, 3, 4] = float("nan")
    step.step(bad, fx["pa"].cuda(), fx["cf_pa"].cuda(), pcf)
    st = step.stats()
    assert st["n_bad"] == 1 and st["skipped_last"] and st["opt_steps"] == 1 and st["n_skipped"] == 1
    after = _snapshot(model, step)
    after["res"] = before["res"]
    _same(before, after)
    assert torch.equal(_bits(step.sums[:6]), _bits(sums[:6]))  # the running sums unchanged
    step.step(x, fx["pa"].cuda(), fx["cf_pa"].cuda(), pcf)  # ... and the next good step counts again
    assert step.stats()["opt_steps"] == 2 and step.epoch_stats()["n"] == 2


def test_scalar_head_addend_matches_the_host_composition_and_is_captured():
    """UKBB's predictor scores age from two scalars with a head that sees no image: its term reaches the Lagrangian as a second
    device addend, computed inside the captured step.  Loss and aux_loss against DSCM.forward on the device, replay against eager."""
    from causal_gen_amd import dscm
    from causal_gen_amd.cf_train import CfTrainStep
    from causal_gen_amd.predictor import AnticausalELBO

    name = PAIRS[0][0]
    g = torch.Generator().manual_seed(8)
    r = lambda: torch.rand(3, 1, generator=g) * 1.6 - 0.8  # noqa: E731
    b = lambda: (torch.rand(3, 1, generator=g) < 0.5).float()  # noqa: E731
    pobs = {"sex": b(), "mri_seq": b(), "age": r(), "brain_volume": r(), "ventricle_volume": r()}
    pcf = {k: (1.0 - v if k in ("sex", "mri_seq") else -0.5 * v) for k, v in pobs.items()}
    snaps = []
    for use_graph in (False, True):
        torch.manual_seed(77)
        fx, hpd, m = _build(name)
        fx["cf_pa"] = torch.cat([fx["cf_pa"][:, :1], fx["pa"][:, 1:]], 1)
        x, pa, cf = fx["x"].cuda(), fx["pa"].cuda(), fx["cf_pa"].cuda()
        pred = _predictor("ukbb", 1, 16)
        args = SimpleNamespace(**{**hpd, "parents_x": ["p0", "p1", "p2"], "dataset": "none", "lmbda_init": LMBDA0, "elbo_constraint": EPS_C,
                                  "damping": DAMPING, "beta": BETA, "grad_skip": GRAD_SKIP})
        model = dscm.DSCM(args, _FixedPGM(fx["cf_pa"][:, 0, 0, 0], pcf), pred, m).cuda()
        for p in m.parameters():
            p.requires_grad_(True)
        step = CfTrainStep(model, args, lr=LR, lr_lagrange=LR_LAG, use_graph=use_graph)
        step.t_abduct = T_AB
        if not use_graph:
            obs = {"x": x, **{n: fx["pa"][:, i, 0, 0].cuda() for i, n in enumerate(args.parents_x)}, **{k: v.cuda() for k, v in pobs.items()}}
            # the same Philox state for both evaluations (DSCM.forward, then the step's own forward and backward) and for the steps
            eng = m.engine()
            eng.rng_ptr()
            state = eng.rng.clone()
            out = model(obs, {"p0": None}, AnticausalELBO(), cf_particles=1, t_abduct=T_AB)
            host_loss, host_aux = float(out["loss"].detach()), float(out["aux_loss"].detach())
            eng.rng.copy_(state)
            loss, aux, _, _, _ = step.loss_and_grads(x, pa, cf, pcf)
            print("scalar head: loss", float(loss), host_loss, "aux_loss", float(aux), host_aux)
            assert _close(loss, host_loss, 1e-6, 1e-7) and _close(aux, host_aux, 1e-6, 1e-7)
            eng.rng.copy_(state)
        for _ in range(3):
            out = step.step(x, pa, cf, pcf)
        snaps.append((_snapshot(model, step), out["out3"].clone(), step.stats()))
    (s0, o0, t0), (s1, o1, t1) = snaps
    assert t0["opt_steps"] == t1["opt_steps"] == 3
    assert torch.equal(_bits(o0), _bits(o1))
    _same(s0, s1)


# ------------------------------------------------------------------------------------------------ step_from
def _from_setup(use_graph):
    """The tiny DGauss HVAE (3 parents: thickness, intensity and a foreign column) with the Morpho-MNIST parent SCM and predictor
    over a 13-column table, and a data set without crop or flip freedom (16x16 images, no padding)."""
    from causal_gen_amd import dscm
    from causal_gen_amd.cf_train import CfTrainStep
    from causal_gen_amd.data import DeviceDataset
    from causal_gen_amd.pgm_train import default_columns

    fx, hpd, m = _build(PAIRS[0][0])
    pgm = PC.make_pgm("morpho")
    cols, ncol = default_columns(pgm)
    cols = dict(cols, extra=ncol)
    N = 8
    obs = PC.draw(pgm, N, seed=4)
    g = torch.Generator().manual_seed(21)
    table = torch.zeros(N, ncol + 1)
    for var, c0 in cols.items():
        if var != "extra":
            table[:, c0:c0 + obs[var].shape[1]] = obs[var]
    table[:, ncol] = torch.randn(N, generator=g)
    x_u8 = torch.randint(0, 256, (N, 1, 16, 16), generator=g, dtype=torch.uint8)
    ds = DeviceDataset(x_u8, table, 16, pad=(0, 0), hflip=0.0)
    args = SimpleNamespace(**{**hpd, "parents_x": ["thickness", "intensity", "extra"], "dataset": "none", "lmbda_init": LMBDA0,
                              "elbo_constraint": EPS_C, "damping": DAMPING, "beta": BETA, "grad_skip": GRAD_SKIP})
    pred = _predictor("morphomnist", 1, 16)
    model = dscm.DSCM(args, pgm, pred, m).cuda()
    for p in m.parameters():
        p.requires_grad_(True)
    columns = {k: ((v, 10) if k == "digit" else v) for k, v in cols.items()}
    step = CfTrainStep(model, args, lr=LR, lr_lagrange=LR_LAG, use_graph=use_graph, columns=columns)
    return ds, pgm, cols, ncol + 1, args, model, step


def test_step_from_equals_step_on_the_same_batch():
    from causal_gen_amd.pgm_cf import PgmCounterfactual

    index = torch.tensor([5, 0, 2], device="cuda")
    do_index = torch.tensor([1, 7, 3], device="cuda")
    torch.manual_seed(7)
    ds, pgm, cols, ncol, args, model_a, step_a = _from_setup(False)
    out_a = step_a.step_from(ds, index, do_index=do_index, do_var="thickness")
    snap_a, o3_a = _snapshot(model_a, step_a), out_a["out3"].clone()

    torch.manual_seed(7)
    ds, pgm, cols, ncol, args, model_b, step_b = _from_setup(False)
    batch = ds.batch(index, train=True)
    cfm = PgmCounterfactual(pgm, args, cols, ncol)
    cf, pa, cf_pa = cfm.run(ds.pa, index, ds.pa, do_index, do_vars=["thickness"])
    width = {"thickness": 1, "intensity": 1, "digit": 10}
    cf_obs = {k: cf[:, cols[k]:cols[k] + w].clone() for k, w in width.items()}
    assert torch.equal(_bits(cf_pa[:, 0]), _bits(ds.pa[do_index, cols["thickness"]]))
    out_b = step_b.step(batch["x"], pa.clone(), cf_pa.clone(), cf_obs)
    snap_b = _snapshot(model_b, step_b)
    assert torch.equal(_bits(o3_a), _bits(out_b["out3"]))
    _same(snap_a, snap_b)
    assert step_a.stats()["opt_steps"] == 1


def test_do_var_changes_the_mask_word_not_the_graph():
    index = torch.tensor([5, 0, 2], device="cuda")
    do_index = torch.tensor([1, 7, 3], device="cuda")
    torch.manual_seed(7)
    ds, pgm, cols, ncol, args, model, step = _from_setup(True)
    for it, var in enumerate(("thickness", "intensity", "thickness", "intensity")):
        step.step_from(ds, index, do_index=do_index, do_var=var)
        torch.cuda.synchronize()
        (ent,) = [e for e in step._ents.values()]
        assert int(ent["mask"]) == ent["cfm"].mask_of([var])
        col = cols[var]
        k = args.parents_x.index(var)
        other = 1 - k
        assert torch.equal(_bits(ent["cf_pa"][:, k]), _bits(ds.pa[do_index, col]))  # the intervened parent is the `do` rows' ...
        if var == "intensity":  # ... and thickness, upstream of it, stays the observation (intensity is downstream of thickness)
            assert torch.equal(_bits(ent["cf_pa"][:, other]), _bits(ds.pa[index, cols["thickness"]]))
        assert step.graph_count() == (0 if not step.use_graph else 1)
    assert step.stats()["opt_steps"] == 4 and len(step._ents) == 1
    step.step_from(ds, index)  # the defaults: a random permutation of the batch and a random variable
    assert step.graph_count() == 1 and step.stats()["opt_steps"] == 5


# ------------------------------------------------------------------------------------------------ checkpoint, weight images
@pytest.mark.parametrize("name,kind", PAIRS)
def test_state_dict_round_trip(name, kind):
    torch.manual_seed(31)
    fx, hpd, model_a, step_a, pobs, pcf = _make(name, kind)
    batch = (fx["x"].cuda(), fx["pa"].cuda(), fx["cf_pa"].cuda(), pcf)
    trace_a = []
    for _ in range(3):  # back to back, no host sync in between: the traces are device-side copies, read at the end
        out = step_a.step(*batch)
        trace_a.append(_trace(step_a, out))
    want = _snapshot(model_a, step_a)

    torch.manual_seed(31)
    fx, hpd, model_b, step_b, _, _ = _make(name, kind)
    trace_b = [_trace(step_b, step_b.step(*batch)) for _ in range(2)]
    # two runs from one seed agree step by step (what follows tests the checkpoint alone); a failure here names the first step and
    # the first quantity -- values, gradient, norm -- that differed between two eager runs
    for it, (ta, tb) in enumerate(zip(trace_a, trace_b)):
        for k in ta:
            assert torch.equal(_bits(ta[k]), _bits(tb[k])), (it, k, float((ta[k].double() - tb[k].double()).abs().max()))
    sd = copy.deepcopy(step_b.state_dict())
    assert {"model_state_dict", "ema_model_state_dict", "optimizer_state_dict", "lagrange_opt_state_dict"} <= set(sd)
    assert "lmbda" in sd["model_state_dict"] and any(k.startswith("vae.") for k in sd["model_state_dict"])

    torch.manual_seed(99)  # (another seed: the noise state must come from the checkpoint)
    fx, hpd, model_c, step_c, _, _ = _make(name, kind)
    step_c.load_state_dict(sd)
    step_c.step(*batch)
    _same(want, _snapshot(model_c, step_c))
    assert step_c.stats()["opt_steps"] == 3 and step_c.it == 3


def test_models_serve_counterfactuals_with_the_updated_weights():
    from causal_gen_amd import dscm as D

    name, kind = PAIRS[0]
    fx, hpd, model, step, pobs, pcf = _make(name, kind)
    x, pa, cf = fx["x"].cuda(), fx["pa"].cuda(), fx["cf_pa"].cuda()

    def serve(vae):
        eng = vae.engine()
        eng.rng_ptr()
        eng.rng.copy_(torch.tensor([1234, 0], dtype=torch.int64))
        return D.counterfactual(vae, x, pa, cf).clone()

    before = [serve(v) for v in (model.vae, step.ema_vae)]  # (builds both engines' weight images)
    step.step(x, pa, cf, pcf)
    after = [serve(v) for v in (model.vae, step.ema_vae)]
    for vae, b, a in zip((model.vae, step.ema_vae), before, after):
        assert not torch.equal(a, b)
        _, _, fresh = _build(name)
        fresh.load_state_dict({k: v.clone() for k, v in vae.state_dict().items()})
        assert torch.equal(_bits(serve(fresh.cuda().eval())), _bits(a))
    assert step.ema_model.vae is step.ema_vae and step.ema_model.predictor is model.predictor
