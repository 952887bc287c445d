"""``cf_train.CfTrainStep`` for mimic: a ``ChestPredictor`` behind the step's predictor seam and ``ChestPGM``'s Gumbel-max uniforms
drawn from the step's own Philox state, on the fixture of tests/chest_cf_fixture.py (32 x 32 pixels, B = 3 and 2).

Against the host composition (``DSCM.forward(..., AnticausalELBO()).backward()`` on the device, same injected noise, same
counterfactual parents): the same kernels in the same order, so the bound is 0 -- equality of every parameter gradient.

Against the f64 oracle (oracle/dscm_ref.dscm_forward in f64 with aux_fn = tests/resnet_ref.chest_ref's loss / B, its ReLU masks
and pool indices pinned to the device's, as tests/test_gpu_predictor_resnet.py pins them): the bounds the CNN pairs are held to in
tests/test_gpu_cf_train_step.py -- values 2e-4 |ref| + 1e-5, the multiplier's gradient 1e-4 |ref| + 1e-6, every parameter gradient
5e-3 of its largest element and 2e-3 in L2.  The test prints the measured figures and, next to them, the yardstick: the same
pinned oracle evaluated by torch in f32 on the CPU against its f64 self.

Steps that are compared bit for bit are taken with ``grad_skip`` = 1e5 (the oracle's gradient norm is 157) and ``n_skipped == 0`` is
asserted with them: a silently dropped step would pass any bit comparison."""
import copy
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import chest_cf_fixture as FX
from chest_cf_fixture import bits
from resnet_ref import chest_ref

pytestmark = pytest.mark.gpu

HOST_BOUND = 0.0
INDEX, DO_INDEX = [5, 0, 2], [1, 7, 3]


def _expand(t, dtype=torch.float32):
    return t[..., None, None].repeat(1, 1, 32, 32).to(dtype)


def _oracle(hp, sd_vae, sd_pred, x, pa_c, cf_c, cf, noise, dtype, masks=None, pool_idx=None):
    """(result dict, state dict with gradients, the multiplier) of the CPU oracle in `dtype`."""
    from oracle import dscm_ref

    B = x.shape[0]
    sd = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in sd_vae.items()}
    lm = torch.tensor([FX.LMBDA0], dtype=dtype, requires_grad=True)
    aux_fn = lambda c: chest_ref(sd_pred, dict(cf, x=c), 0.0, masks=masks, pool_idx=pool_idx, dtype=dtype)["loss"] / B  # noqa: E731
    ref = dscm_ref.dscm_forward(sd, SimpleNamespace(**vars(hp)), x.to(dtype), _expand(pa_c, dtype), [_expand(cf_c, dtype)], hp.beta, t_abduct=1.0,
                                noise=noise, aux_fn=aux_fn, lmbda=lm, eps=torch.tensor([FX.EPS_C], dtype=dtype), damping=FX.DAMPING)
    ref["loss"].sum().backward()
    return ref, sd, lm


@functools.lru_cache(maxsize=None)
def _case():
    """One device evaluation with injected noise, by the host composition and by the step, shared by the two comparisons."""
    from causal_gen_amd.predictor import AnticausalELBO
    from oracle import hvae_ref

    f = FX.make()
    m, step, model = f.vae, f.step, f.model
    cpu = lambda d: {k: v.cpu() for k, v in d.items()}  # noqa: E731
    sd_vae = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    sd_pred = {k: v.detach().cpu().clone() for k, v in f.pred.state_dict().items()}
    # the noise, in the reference's draw order: an f32 run of the free oracle on the CPU draws and records it
    noise = hvae_ref._Noise(None)
    torch.manual_seed(17)
    _oracle(f.hp, sd_vae, sd_pred, f.x.cpu(), f.pa_c.cpu(), f.cf_c.cpu(), cpu(f.cf), noise, torch.float32)
    drawn = [e.clone() for e in noise.drawn]

    m.noise = [e.clone() for e in drawn]
    out = model(dict(f.pa, x=f.x), {"sex": None}, AnticausalELBO(), cf_particles=1, t_abduct=1.0)
    assert not m.noise
    out["loss"].sum().backward()
    torch.cuda.synchronize()
    host = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    host_lm, host_loss = float(model.lmbda.grad), float(out["loss"].detach())
    pred_grads_none = all(p.grad is None for p in f.pred.parameters())

    m.noise = [e.clone() for e in drawn]
    loss, aux, out3, g_l, grads = step.loss_and_grads(f.x, f.pa_c, f.cf_c, f.cf)
    torch.cuda.synchronize()
    assert not m.noise
    (ent,) = step._ents.values()
    acts = [a.cpu() for a in f.pred.trunk_activations()]  # what the step's forward left in the predictor's workspace
    return SimpleNamespace(f=f, sd_vae=sd_vae, sd_pred=sd_pred, drawn=drawn, host=host, host_lm=host_lm, host_loss=host_loss,
                           pred_grads_none=pred_grads_none, loss=loss, aux=aux, out3=out3, g_l=g_l, grads=grads, acts=acts,
                           cf_x=ent["cf_x"].detach().cpu().clone(), terms=ent["terms"].cpu().clone())


def test_loss_and_grads_equal_the_host_composition():
    c = _case()
    f = c.f
    worst, checked = 0.0, 0
    for n_, g in c.host.items():
        assert n_ in c.grads, n_
        if float(g.abs().max()) == 0.0:
            continue
        worst = max(worst, float((c.grads[n_] - g).abs().max()) / float(g.abs().max()))
        checked += 1
    print(f"chest: device step against DSCM.forward.backward over {checked} gradients: worst relative-to-max deviation {worst:.3e}, "
          f"loss {float(c.loss)!r} against {c.host_loss!r}, g_lmbda {float(c.g_l)!r} against {c.host_lm!r}")
    assert checked > 20 and set(c.grads) == set(c.host)
    assert worst <= HOST_BOUND
    assert abs(float(c.loss) - c.host_loss) <= 1e-6 * abs(c.host_loss) and abs(float(c.g_l) - c.host_lm) <= 1e-6 * abs(c.host_lm)
    # the predictor is frozen: no gradient, the same bits
    assert c.pred_grads_none and all(p.grad is None for p in f.pred.parameters())
    for k, v in f.pred.state_dict().items():
        assert torch.equal(v.cpu(), c.sd_pred[k]), k
    assert tuple(c.terms.shape) == (3, 4) and abs(float(c.terms.double().sum()) / 3 - float(c.aux)) <= 1e-5 * abs(float(c.aux))
    assert f.step.epoch_stats()["n"] == 0  # loss_and_grads leaves the running sums alone


def test_loss_and_grads_match_the_f64_oracle_with_pinned_masks():
    """Measured on gfx950 (B = 3, 32 x 32; LABNOTES 40): 180 parameter gradients, worst 2.8e-5 of a gradient's largest element and
    1.3e-5 in L2 (bounds 5e-3 / 2e-3); the same pinned oracle in f32 on the CPU against its f64 self: 3.0e-5 / 8.8e-6.  loss
    209.32410 against 209.32432, d loss / d lmbda 4.3771815 against 4.3771839; no pinned ReLU or pool decision disagreed."""
    from oracle import hvae_ref

    c = _case()
    f = c.f
    cpu = lambda d: {k: v.cpu() for k, v in d.items()}  # noqa: E731
    masks = [(a > 0).double() for a in c.acts[:17]]
    pool_idx = F.max_pool2d(c.acts[0], 3, 2, 1, return_indices=True)[1]
    args = (f.hp, c.sd_vae, c.sd_pred, f.x.cpu(), f.pa_c.cpu(), f.cf_c.cpu(), cpu(f.cf))
    ref, sd, lm = _oracle(*args, hvae_ref._Noise([e.double() for e in c.drawn]), torch.float64, masks, pool_idx)
    r32, sd32, lm32 = _oracle(*args, hvae_ref._Noise([e.clone() for e in c.drawn]), torch.float32, [m_.float() for m_ in masks], pool_idx)

    # the pinning is legitimate: on the image the device's predictor saw, a unit whose mask differs from the free f64 oracle's has
    # a free pre-activation within the activation tolerance of zero (tests/test_gpu_predictor_resnet.py's rule and tolerance)
    with torch.no_grad():
        obs = dict(cpu(f.cf), x=c.cf_x)
        free = chest_ref(c.sd_pred, obs, 0.0)
        free32 = chest_ref(c.sd_pred, obs, 0.0, dtype=torch.float32)
    rel = lambda a, b: float((a.double() - b.double()).abs().max()) / max(float(b.abs().max()), 1e-30)  # noqa: E731
    tol = [max(1e-5, 4 * rel(a, b)) for a, b in zip(free32["acts"], free["acts"])]
    flips = 0
    for i, (mk, pre, act) in enumerate(zip(masks, free["pres"], free["acts"])):
        diff = mk != (pre > 0).double()
        if bool(diff.any()):
            flips += int(diff.sum())
            assert float(pre[diff].abs().max()) <= tol[i] * float(act.abs().max()), (i, int(diff.sum()), float(pre[diff].abs().max()))
    free_idx = F.max_pool2d(free["acts"][0], 3, 2, 1, return_indices=True)[1]
    pool_diff = pool_idx != free_idx
    if bool(pool_diff.any()):
        stem = free["acts"][0].flatten(2)
        gap = (stem.gather(2, free_idx.flatten(2)) - stem.gather(2, pool_idx.flatten(2))).abs()
        assert float(gap.max()) <= tol[0] * float(stem.abs().max())
    for i, (got, want) in enumerate(zip(c.acts, free["acts"])):
        assert rel(got, want) <= tol[i], (i, rel(got, want), tol[i])

    val = lambda r, k: float(r[k].detach().reshape(-1)[0])  # noqa: E731
    bad = []
    for got, key in ((c.loss, "loss"), (c.aux, "aux_loss"), (c.out3[0], "elbo"), (c.out3[1], "nll"), (c.out3[2], "kl")):
        want = val(ref, key)
        print(f"chest {key}: device {float(got)!r}, f64 oracle {want!r}, f32 oracle {val(r32, key)!r}")
        if not abs(float(got) - want) <= 2e-4 * abs(want) + 1e-5:
            bad.append((key, float(got), want))
    print(f"chest g_lmbda: device {float(c.g_l)!r}, f64 oracle {float(lm.grad)!r}, f32 oracle {float(lm32.grad)!r}")
    if not abs(float(c.g_l) - float(lm.grad)) <= 1e-4 * abs(float(lm.grad)) + 1e-6:
        bad.append(("g_lmbda", float(c.g_l), float(lm.grad)))
    checked, worst, worst32 = 0, [0.0, 0.0, ""], [0.0, 0.0]
    for n_ in c.sd_vae:
        rg = sd[n_].grad
        if rg is None or float(rg.abs().max()) == 0.0:
            continue
        g = c.grads[n_].cpu().double()
        d, l2 = float((g - rg).abs().max()) / float(rg.abs().max()), float((g - rg).norm()) / float(rg.norm())
        g32 = sd32[n_].grad.double()
        worst32 = [max(worst32[0], float((g32 - rg).abs().max()) / float(rg.abs().max())), max(worst32[1], float((g32 - rg).norm()) / float(rg.norm()))]
        if d > worst[0]:
            worst = [d, max(worst[1], l2), n_]
        worst[1] = max(worst[1], l2)
        if not (d < 5e-3 and l2 < 2e-3):
            bad.append((n_, d, l2))
        checked += 1
    print(f"chest: {checked} parameter gradients against the pinned f64 oracle: worst max-norm {worst[0]:.3e} ({worst[2]}), worst L2 {worst[1]:.3e}; "
          f"the f32 oracle against its f64 self: {worst32[0]:.3e} / {worst32[1]:.3e}; pinned ReLU disagreements {flips}, "
          f"pool disagreements {int(pool_diff.sum())}")
    assert checked > 20
    assert not bad, bad


def _batch(f):
    return f.x, f.pa_c, f.cf_c, f.cf


def test_graph_replay_equals_eager_for_two_batch_shapes():
    outs = []
    for use_graph in (False, True):
        torch.manual_seed(123)
        f = FX.make(use_graph=use_graph)
        f2 = FX.parts(B=2)  # the second batch shape: a second static entry and a second graph
        pa2, x2 = f2[4], f2[5]
        cf2 = FX.cf_of(pa2)
        small = (x2.cuda(), FX.compact(f.hp, pa2).cuda(), FX.compact(f.hp, cf2).cuda(), {k: v.cuda() for k, v in cf2.items()})
        first = None
        for it in range(4):
            out = f.step.step(*_batch(f))
            if first is None:  # (the call that captures returns this step's values, not the graph's unwritten output)
                first = torch.stack([out["elbo"], out["nll"], out["kl"], out["loss"], out["aux_loss"]]).clone(), out["out3"].clone()
            if it == 1:
                for _ in range(2):
                    o2 = f.step.step(*small)
                small_out = o2["out3"].clone()
        outs.append((out["out3"].clone(), FX.snapshot(f.model, f.step), f.step.stats(), f.step.graph_count(), first, small_out))
    (o0, s0, t0, g0, f0, m0), (o1, s1, t1, g1, f1, m1) = outs
    assert t0["opt_steps"] == t1["opt_steps"] == 6 and t0["n_skipped"] == t1["n_skipped"] == 0 and t0["n_bad"] == t1["n_bad"] == 0
    assert (g0, g1) == (0, 2)
    assert torch.equal(bits(f0[0]), bits(f1[0])) and torch.equal(bits(f0[1]), bits(f1[1])), (f0, f1)
    assert bool(torch.isfinite(f1[1]).all()) and torch.equal(bits(f1[0][:3]), bits(f1[1]))
    assert torch.equal(bits(o0), bits(o1)) and torch.equal(bits(m0), bits(m1))
    FX.same(s0, s1)
    assert t0["lmbda"] == t1["lmbda"] != FX.LMBDA0
    assert float(s0["sums"][5]) == 6.0


def test_skip_and_nan_leave_everything_untouched():
    f = FX.make(grad_skip=1e-6)  # every step is "too large"
    before = FX.snapshot(f.model, f.step)
    for _ in range(2):
        f.step.step(*_batch(f))
    st = f.step.stats()
    assert st["n_skipped"] == 2 and st["opt_steps"] == 0 and st["skipped_last"] and st["n_bad"] == 0
    FX.same(before, FX.snapshot(f.model, f.step), skip=("res", "sums"))  # (the step's own results and statistics are written)
    assert f.step.epoch_stats()["n"] == 2

    f = FX.make()
    f.step.step(*_batch(f))
    before, sums = FX.snapshot(f.model, f.step), f.step.sums.clone()
    bad = f.x.clone()
    bad[1, 0, 3, 4] = float("nan")
    f.step.step(bad, f.pa_c, f.cf_c, f.cf)
    st = f.step.stats()
    assert st["n_bad"] == 1 and st["skipped_last"] and st["opt_steps"] == 1 and st["n_skipped"] == 1
    FX.same(before, FX.snapshot(f.model, f.step), skip=("res", "sums"))
    assert torch.equal(bits(f.step.sums[:6]), bits(sums[:6]))
    f.step.step(*_batch(f))
    assert f.step.stats()["opt_steps"] == 2 and f.step.epoch_stats()["n"] == 2


def test_a_larger_call_between_steps_leaves_the_captured_workspace_alone():
    """``ChestPredictor`` caches one workspace and replaces it when a larger call arrives; the step's record keeps the one its
    graph was captured over, and ``trunk_activations()`` reads the workspace of the last forward, whichever record ran it."""
    from resnet_ref import make_obs

    runs = []
    for disturb in (False, True):
        torch.manual_seed(5)
        f = FX.make(B=2, use_graph=True)
        for it in range(3):
            f.step.step(*_batch(f))
            if disturb and it == 0:
                (ent,) = f.step._ents.values()
                held = ent["plan"]["run"]["ws"]
                assert f.pred.__dict__["_ws"] is held
                f.pred.nll_terms(**{k: v.cuda() for k, v in make_obs(5, 32, 9).items()})  # five images: a larger workspace
                assert f.pred.__dict__["_ws"] is not held and f.pred.__dict__["_ws"].numel() > held.numel()
                assert f.pred.trunk_activations()[0].shape[0] == 5
        acts = f.pred.trunk_activations()
        assert acts[0].shape[0] == 2 and len(acts) == 18
        st = f.step.stats()
        assert st["opt_steps"] == 3 and st["n_skipped"] == 0 and f.step.graph_count() == 1
        runs.append((FX.snapshot(f.model, f.step), acts))
    FX.same(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ step_from
def _cf_table(step):
    (ent,) = step._ents.values()
    return ent["cfm"]._entry(ent["B"])["cf"]


@pytest.mark.parametrize("var", ["sex", "race", "age", "finding"])
def test_step_from_equals_step_on_the_same_batch(var):
    from causal_gen_amd.pgm_cf import PgmCounterfactual

    index, do_index = torch.tensor(INDEX, device="cuda"), torch.tensor(DO_INDEX, device="cuda")
    torch.manual_seed(7)
    fa = FX.make(pgm="scm")
    ds, _ = FX.dataset()
    out_a = fa.step.step_from(ds, index, do_index=do_index, do_var=var)
    snap_a, o3_a, cf_a = FX.snapshot(fa.model, fa.step), out_a["out3"].clone(), _cf_table(fa.step).clone()

    torch.manual_seed(7)
    fb = FX.make(pgm="scm")
    ds, _ = FX.dataset()
    batch = ds.batch(index, train=True)
    cfm = PgmCounterfactual(fb.scm, fb.hp)
    eng = fb.step.eng
    eng.rng_ptr()  # the Philox state the step will see: the counterfactual launch reads it before the step's advance
    drawn = var in ("age", "finding")  # (sex and race are not upstream of finding: nothing drawn is used)
    cf, pa, cf_pa = cfm.run(ds.pa, index, ds.pa, do_index, do_vars=[var], rng=eng.rng if drawn else None)
    cf_obs = {k: cf[:, c0:c0 + FX.WIDTH[k]].clone() for k, c0 in FX.COLUMNS.items()}
    c0, w = FX.COLUMNS[var], FX.WIDTH[var]
    assert torch.equal(bits(cf[:, c0:c0 + w]), bits(ds.pa[do_index, c0:c0 + w]))
    out_b = fb.step.step(batch["x"], pa.clone(), cf_pa.clone(), cf_obs)
    snap_b = FX.snapshot(fb.model, fb.step)
    assert torch.equal(bits(cf_a), bits(cf))
    assert torch.equal(bits(o3_a), bits(out_b["out3"]))
    FX.same(snap_a, snap_b)
    st = fa.step.stats()
    assert st["opt_steps"] == 1 and st["n_skipped"] == 0 and fb.step.stats()["n_skipped"] == 0


def test_do_var_changes_the_mask_word_not_the_graph():
    index, do_index = torch.tensor(INDEX, device="cuda"), torch.tensor(DO_INDEX, device="cuda")
    torch.manual_seed(7)
    f = FX.make(use_graph=True, pgm="scm")
    ds, _ = FX.dataset()
    step = f.step
    order = ("sex", "race", "age", "finding", "race", "age", "finding", "sex")
    for var in order:
        step.step_from(ds, index, do_index=do_index, do_var=var)
        torch.cuda.synchronize()
        (ent,) = step._ents.values()
        assert int(ent["mask"]) == ent["cfm"].mask_of([var])
        cf = _cf_table(step)
        c0, w = FX.COLUMNS[var], FX.WIDTH[var]
        assert torch.equal(bits(cf[:, c0:c0 + w]), bits(ds.pa[do_index, c0:c0 + w])), var  # race: three columns
        assert bool(((cf[:, 4] == 0) | (cf[:, 4] == 1)).all())
        if var in ("sex", "race"):  # not upstream of anything: every other column is the observation's
            keep = [c for c in range(6) if not c0 <= c < c0 + w]
            assert torch.equal(bits(cf[:, keep]), bits(ds.pa[index][:, keep])), var
        k = {"age": slice(0, 1), "race": slice(1, 4), "sex": slice(4, 5), "finding": slice(5, 6)}[var]  # args.parents_x order
        assert torch.equal(bits(ent["cf_pa"][:, k]), bits(ds.pa[do_index, c0:c0 + w]))
        assert step.graph_count() == 1
    st = step.stats()
    assert st["opt_steps"] == len(order) and st["n_skipped"] == 0 and len(step._ents) == 1
    step.step_from(ds, index)  # the defaults: a random permutation of the batch and a random variable
    assert step.graph_count() == 1 and step.stats()["opt_steps"] == len(order) + 1


# ------------------------------------------------------------------------------------------------ the draws belong to the step
def _trace(step, out):
    """Device-side copies (no host sync) of what a step computed: its values, the counterfactual table, the gradient, the tail's state."""
    return {"out3": out["out3"].clone(), "res": step.res.clone(), "cf": _cf_table(step).clone(), "flat_g": step.eng.flat_g.clone(),
            "state": step.state.clone()}


def _same_traces(ta, tb):
    """Names the first step and the first quantity that differs between two runs (LABNOTES 36.5's protocol)."""
    for it, (a, b) in enumerate(zip(ta, tb)):
        for k in a:
            assert torch.equal(bits(a[k]), bits(b[k])), (it, k, float((a[k].double() - b[k].double()).abs().max()))


def _run_from(seed, do_vars, disturb=False, use_graph=True):
    index, do_index = torch.tensor(INDEX, device="cuda"), torch.tensor(DO_INDEX, device="cuda")
    torch.manual_seed(seed)
    f = FX.make(use_graph=use_graph, pgm="scm")
    ds, _ = FX.dataset()
    trace = []
    for var in do_vars:
        if disturb:
            torch.rand(7, device="cuda")  # torch's CUDA generator moves on: none of the step's business
        trace.append(_trace(f.step, f.step.step_from(ds, index, do_index=do_index, do_var=var)))
    return f, ds, trace


def test_torchs_generator_does_not_decide_the_counterfactual_finding():
    fa, _, ta = _run_from(31, ["age"] * 3)
    fb, _, tb = _run_from(31, ["age"] * 3, disturb=True)
    _same_traces(ta, tb)
    FX.same(FX.snapshot(fa.model, fa.step), FX.snapshot(fb.model, fb.step))
    for f in (fa, fb):
        st = f.step.stats()
        assert st["opt_steps"] == 3 and st["n_skipped"] == 0 and st["n_bad"] == 0 and f.step.graph_count() == 1
    assert int(fa.step.eng.rng[1]) == int(fb.step.eng.rng[1]) == 3  # one advance per step; the uniforms advance nothing


def test_state_dict_round_trip_continues_the_gumbel_draws():
    index, do_index = torch.tensor(INDEX, device="cuda"), torch.tensor(DO_INDEX, device="cuda")
    order = ["age", "age", "finding"]
    fa, ds, ta = _run_from(31, order)
    want = FX.snapshot(fa.model, fa.step)
    fb, ds_b, tb = _run_from(31, order[:2], disturb=True)
    _same_traces(ta[:2], tb)  # two runs from one seed agree step by step: what follows tests the checkpoint alone
    sd = copy.deepcopy(fb.step.state_dict())
    assert sd["cgen"]["rng"] is not None and int(sd["cgen"]["rng"][1]) == 2

    fc, ds_c, _ = _run_from(99, [])  # (another seed: the Philox state must come from the checkpoint)
    fc.step.load_state_dict(sd)
    out = fc.step.step_from(ds_c, index, do_index=do_index, do_var="finding")
    _same_traces(ta[2:], [_trace(fc.step, out)])
    FX.same(want, FX.snapshot(fc.model, fc.step))
    st = fc.step.stats()
    assert st["opt_steps"] == 3 and fc.step.it == 3 and st["n_skipped"] == 0


def test_models_serve_counterfactuals_with_the_updated_weights():
    from causal_gen_amd import dscm as D
    from causal_gen_amd.predictor import AnticausalELBO

    f = FX.make()
    step, model = f.step, f.model
    obs = dict(f.pa, x=f.x)
    pa4, cf4 = (t[..., None, None].expand(-1, -1, 32, 32) for t in (f.pa_c, f.cf_c))
    pred_bits = {k: v.clone() for k, v in f.pred.state_dict().items()}

    def serve(dscm_model):
        eng = dscm_model.vae.engine()
        eng.rng_ptr()
        eng.rng.copy_(torch.tensor([1234, 0], dtype=torch.int64))
        with torch.no_grad():
            out = dscm_model(obs, {"sex": None}, AnticausalELBO())
            cfx = D.counterfactual(dscm_model.vae, f.x, pa4, cf4)
        return out["cfs"]["x"].clone(), out["aux_loss"].clone(), out["loss"].clone(), cfx.clone()

    models = (model, step.ema_model)
    before = [serve(mm) for mm in models]  # (builds both engines' weight images)
    step.step(*_batch(f))
    assert step.stats()["opt_steps"] == 1
    after = [serve(mm) for mm in models]
    for mm, b, a in zip(models, before, after):
        assert not torch.equal(a[0], b[0]) and not torch.equal(a[3], b[3])
        assert all(bool(torch.isfinite(t).all()) for t in a)
        hp, fresh, _, _, _, _ = FX.parts()
        fresh.load_state_dict({k: v.clone() for k, v in mm.vae.state_dict().items()})
        twin = D.DSCM(hp, model.pgm, f.pred, fresh.cuda().eval()).cuda()
        twin.lmbda.data = mm.lmbda.data.clone()
        for got, want in zip(serve(twin), a):
            assert torch.equal(bits(got), bits(want))
    assert step.ema_model.vae is step.ema_vae and step.ema_model.predictor is model.predictor is f.pred
    assert all(p.grad is None for p in f.pred.parameters())
    for k, v in f.pred.state_dict().items():
        assert torch.equal(v, pred_bits[k]), k
