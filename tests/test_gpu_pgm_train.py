"""Training the parent SCMs on the MI355X (causal_gen_amd.pgm_train.PgmTrainStep over csrc/pgm.hip): terms, loss and every
parameter gradient of the four PGMs against the host density ``pgm.log_prob`` in f64 with autograd, determinism, the optimiser
trajectory against a host AdamW / LambdaLR / clip / EMA loop, NaN skip, the gathered step, the checkpoint round trip and a fit.

Bounds.  Nothing is fixed in advance.  For every compared tensor the test measures e32, the deviation of the SAME host code run
in f32 on the CPU from the f64 oracle -- absolute for terms and the loss (relative to max(1, |oracle|)), relative to the largest
entry of the oracle's tensor for a gradient -- and holds the kernel to 4 * max(e32, 2^-24): the kernel sums in another order than
torch and its erff / expf are not torch's; 2^-24 is what rounding the f64 oracle itself to f32 costs, so a lucky e32 = 0 on a
one-element tensor does not ask for more than the format holds.  A gradient tensor that is exactly zero in the oracle (a spline
whose every row lies outside the bound) must be exactly zero.
On a knot of the spline the gradient with respect to the heights is discontinuous (the jump is [f''] / f'^2 * d knot / d height),
and whether an f32 input is "on" a knot is decided by the precision the knot was computed in.  The knot rows are the f32 host
module's own knots; the f64 oracle and the kernel, which derives the knots in f64 from the same f32 parameters, bin them alike.
The clamp rows (Morpho-MNIST observations at +-1 and +-(1 - 1e-7)) saturate torch's SigmoidTransform clamp, which is the
dtype's: f32 and f64 differ there by design, e32 is large and the oracle bound says little; those rows are additionally held to
the f32 host run itself at 1e-3 (a wrong clamp constant moves u from -87.3 to -103 or to -16: tens of percent).

Measured on the MI355X (every case prints its figures; LABNOTES 19).  Host f32 against f64, over the 22 shape cases and the
outside-the-bound and knot batches: terms median 6.8e-8 (1.4e-9 .. 2.2e-4, the largest on a knot row of ChestPGM's 8-bin spline),
loss median 7.2e-8 (up to 1.5e-5), gradients median 3.1e-7 relative to the tensor's largest entry (0 .. 3e-5 on the shape cases; on
the knot batches the f32 host bins rows on the other side of a knot and misses the heights by 0.9 .. 2.9 of the largest entry).  The
bounds are therefore 2.4e-7 (the floor) .. 8.8e-4 for terms, 2.4e-7 .. 5.9e-5 for the loss, 2.4e-7 .. 1.2e-4 for gradients off the
knots.  The kernel: terms <= 1.6e-7 (median 3.8e-8), loss <= 8.5e-8, gradients median 5.9e-8, at most 0.60 of its bound anywhere.
Trajectory (25 steps, lr 1e-3): host f32 against host f64 3.2e-7 .. 5.1e-7 on the parameters, 1.3e-7 .. 3.1e-7 on the losses,
2.2e-6 .. 7.9e-6 on the norms, hence bounds of 1.3e-6 .. 2.0e-6, 5.1e-7 .. 1.2e-6 and 8.8e-6 .. 3.2e-5; the kernel stays at
4.2e-7 .. 6.8e-7, 1.0e-7 and 1.1e-6 .. 1.8e-6.  Fit: see test_a_fit_recovers_the_generating_model."""
import copy
import functools
import math
from types import SimpleNamespace

import pytest
import torch

import pgm_cases as PC
from oracle import train_ref

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -24
FACTOR = 4.0

# tag: (kind, hidden widths or None for the PGM's own, rows, edge rows?)   64 rows = one workgroup = one wave
CASES = {}
for _k in PC.KINDS:
    for _b in (1, 2, 65, 129):
        CASES[f"{_k}_b{_b}"] = (_k, None, _b)
for _k in ("flow", "morpho"):  # context dimension 2 and 1; the PGMs' own widths are [32, 32] (flow, morpho) and [8, 16] (chest)
    for _w in ([8, 16], [64], [64, 64, 64]):
        CASES[f"{_k}_w{'x'.join(map(str, _w))}"] = (_k, _w, 65)


def _step_cls():
    from causal_gen_amd.pgm_train import PgmTrainStep

    return PgmTrainStep


def _bits(t):
    return t.contiguous().view(torch.int32)


def host_eval(m, obs, dtype):
    """terms [B, mechanisms], mean loss and every parameter gradient of `m.nll`, on the CPU in `dtype`."""
    mm = copy.deepcopy(m).cpu().to(dtype)
    o = {k: v.cpu().to(dtype) for k, v in obs.items()}
    lp = mm.log_prob(o)
    terms = torch.stack([lp[mech.var] for mech in mm.mechanisms()], 1)
    loss = mm.nll(o)
    grads = torch.autograd.grad(loss, list(mm.parameters()), allow_unused=True)
    names = [n for n, _ in mm.named_parameters()]
    return dict(terms=terms.detach().double(), loss=loss.detach().double(),
                grads={n: (torch.zeros_like(p) if g is None else g).double() for n, g, p in zip(names, grads, mm.parameters())})


def deviations(got, ref):
    """{tensor name: deviation of `got` from the oracle `ref`}: terms per mechanism column and the loss relative to
    max(1, |oracle|), a gradient relative to its oracle's largest entry (absolute if the oracle is all zero)."""
    out = {}
    for j in range(ref["terms"].shape[1]):
        r = ref["terms"][:, j]
        out[f"terms[{j}]"] = ((got["terms"][:, j].double() - r).abs() / r.abs().clamp_min(1.0)).max().item()
    out["loss"] = abs(got["loss"].double().item() - ref["loss"].item()) / max(1.0, abs(ref["loss"].item()))
    for n, r in ref["grads"].items():
        scale = r.abs().max().item()
        out["grad " + n] = (got["grads"][n].double().cpu() - r).abs().max().item() / (scale if scale > 0 else 1.0)
    return out


def kernel_eval(m, obs):
    ts = _step_cls()(copy.deepcopy(m), ema=False, use_graph=False)
    dobs = {k: v.cuda() for k, v in obs.items()}
    terms = ts.terms(**dobs)
    l_fwd = ts.loss(**dobs)
    loss, grads = ts.loss_and_grads(**dobs)
    B = terms.shape[0]
    assert torch.equal(_bits(terms), _bits(ts._statics[("obs", B)]["terms"]))  # the forward of both entry points is one code
    assert torch.equal(_bits(l_fwd), _bits(loss))
    torch.cuda.synchronize()
    return dict(terms=terms.cpu(), loss=loss.cpu(), grads={k: v.cpu() for k, v in grads.items()}), ts


@functools.lru_cache(maxsize=None)
def _case(tag):
    kind, widths, B = CASES[tag]
    m = PC.make_pgm(kind, seed=0, widths=widths)
    obs = PC.draw(m, B, seed=B)
    if B >= 65:
        obs = PC.edge_rows(m, obs, kind)
    return m, obs, host_eval(m, obs, torch.float64), host_eval(m, obs, torch.float32)


def _hold(tag, errs, e32, exact_zero=()):
    miss = {}
    for n in errs:
        bound = FACTOR * max(e32[n], FLOOR)
        print(f"{tag} {n}: kernel {errs[n]:.3e}  host f32 {e32[n]:.3e}  bound {bound:.3e}")
        if n in exact_zero:
            if errs[n] != 0.0:
                miss[n] = (errs[n], 0.0)
        elif not errs[n] <= bound:
            miss[n] = (errs[n], bound)
    assert not miss, (tag, miss)


@pytest.mark.parametrize("tag", sorted(CASES))
def test_terms_loss_and_gradients_match_the_f64_host_density(tag):
    m, obs, r64, r32 = _case(tag)
    got, _ = kernel_eval(m, obs)
    assert set(got["grads"]) == set(r64["grads"]) and got["terms"].shape == r64["terms"].shape
    zero = {"grad " + n for n, g in r64["grads"].items() if g.abs().max().item() == 0.0}
    _hold(tag, deviations(got, r64), deviations(r32, r64), exact_zero=zero)


@pytest.mark.parametrize("kind", ("flow", "chest"))
def test_rows_outside_the_bound_leave_the_spline_parameters_at_exact_zero(kind):
    m = PC.make_pgm(kind, seed=5)
    obs = PC.outside_rows(m)
    r64, r32 = host_eval(m, obs, torch.float64), host_eval(m, obs, torch.float32)
    got, _ = kernel_eval(m, obs)
    spline = [n for n in r64["grads"] if "unnormalized_" in n]
    assert len(spline) == 4
    for n in spline:
        assert r64["grads"][n].abs().max().item() == 0.0 and bool((got["grads"][n] == 0).all()), n
    _hold(kind + "_outside", deviations(got, r64), deviations(r32, r64), exact_zero={"grad " + n for n in spline})


@pytest.mark.parametrize("kind", ("flow", "morpho", "chest"))
def test_rows_on_the_interior_knots(kind):
    m = PC.make_pgm(kind, seed=11)
    rows = PC.knot_rows(m)
    assert len(rows) == PC.spline_of(m).count_bins - 1
    obs = {k: torch.cat([r[k] for r in rows]) for k in rows[0]}
    if not PC.spline_var(m).normalize:  # (the rows ARE the f32 module's knots: it bins every one of them upwards, at theta = 0)
        with torch.no_grad():
            assert torch.equal(PC.spline_of(m)._knots()[1][0, 1:-1], obs[PC.spline_var(m).var][:, 0])
    r64, r32 = host_eval(m, obs, torch.float64), host_eval(m, obs, torch.float32)
    got, _ = kernel_eval(m, obs)
    _hold(kind + "_knots", deviations(got, r64), deviations(r32, r64))


def test_morpho_rows_at_the_clamp_of_the_normalisation():
    m = PC.make_pgm("morpho", seed=13)
    obs = PC.clamp_rows(m)
    r64, r32 = host_eval(m, obs, torch.float64), host_eval(m, obs, torch.float32)
    got, _ = kernel_eval(m, obs)
    assert bool(torch.isfinite(got["terms"]).all()) and all(bool(torch.isfinite(g).all()) for g in got["grads"].values())
    _hold("morpho_clamp", deviations(got, r64), deviations(r32, r64))
    vs32 = deviations(got, {k: (v.double() if k != "grads" else {n: g.double() for n, g in v.items()}) for k, v in r32.items()})
    print("morpho_clamp against the f32 host run:", {k: f"{v:.2e}" for k, v in vs32.items()})
    assert max(vs32.values()) <= 1e-3, vs32


@pytest.mark.parametrize("tag", ("flow_b129", "morpho_w64x64x64", "chest_b65"))
def test_reruns_are_bit_identical(tag):
    m, obs, _, _ = _case(tag)
    runs = []
    for _ in range(2):
        got, ts = kernel_eval(m, obs)
        runs.append((got, ts.flat_g.clone()))
    (a, ga), (b, gb) = runs
    assert torch.equal(_bits(a["terms"]), _bits(b["terms"])) and torch.equal(_bits(a["loss"]), _bits(b["loss"])) and torch.equal(_bits(ga), _bits(gb))


# ----------------------------------------------------------------------------- the optimiser trajectory
HP = dict(lr=1e-3, wd=0.1, betas=(0.9, 0.999), eps=1e-8, grad_clip=200.0, lr_warmup_steps=1, ema_rate=0.999, ema_update_after=2)


def host_loop(m, batches, steps, dtype, hp=HP):
    """sup_epoch on alternating fixed batches: AdamW under LambdaLR(linear_warmup), clip_grad_norm_, the project's EMA rule."""
    mm = copy.deepcopy(m).cpu().to(dtype)
    params = list(mm.parameters())
    ema = [p.detach().clone() for p in params]
    opt = torch.optim.AdamW(params, lr=hp["lr"], weight_decay=hp["wd"], betas=hp["betas"], eps=hp["eps"])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, train_ref.linear_warmup(hp["lr_warmup_steps"]))
    losses, norms = [], []
    for t in range(steps):
        o = {k: v.to(dtype) for k, v in batches[t % len(batches)].items()}
        opt.zero_grad()
        loss = mm.nll(o)
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, hp["grad_clip"])))
        opt.step()
        sched.step()
        losses.append(float(loss))
        d = train_ref.ema_decay(t, hp["ema_rate"], hp["ema_update_after"])
        with torch.no_grad():
            for e, p in zip(ema, params):
                if d is None:
                    e.copy_(p)
                else:
                    e.sub_((e - p) * (1.0 - d))
    flat = lambda ts: torch.cat([t.detach().reshape(-1).double() for t in ts])
    return dict(p=flat(params), ema=flat(ema), loss=torch.tensor(losses, dtype=torch.float64), norm=torch.tensor(norms, dtype=torch.float64)), mm


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


@pytest.mark.parametrize("kind", ("flow", "morpho", "chest"))
def test_twenty_five_steps_follow_the_host_optimiser_loop(kind):
    m = PC.make_pgm(kind, seed=25 if kind == "chest" else 21)  # (seeds at which the host loops agree: asserted below)
    batches = [PC.draw(m, 48, seed=s) for s in (1, 2, 3)]
    h64, _ = host_loop(m, batches, 25, torch.float64)
    h32, _ = host_loop(m, batches, 25, torch.float32)
    runs = {}
    for graph in (True, False):
        ts = _step_cls()(copy.deepcopy(m), use_graph=graph, **HP)
        dev = [{k: v.cuda() for k, v in b.items()} for b in batches]
        outs = [ts.step(**dev[t % 3]) for t in range(25)]
        torch.cuda.synchronize()
        assert bool(ts._graphs) == graph and ts.stats()["opt_steps"] == 25 and ts.stats()["n_skipped"] == 0
        runs[graph] = dict(p=ts._on.flat_p.clone(), ema=ts._ema.flat_p.clone(), loss=torch.stack([o["loss"] for o in outs]),
                           norm=torch.stack([o["grad_norm"] for o in outs]), m=ts.m.clone(), v=ts.v.clone(), state=ts.state.clone())
    for k in runs[True]:
        assert torch.equal(_bits(runs[True][k]), _bits(runs[False][k])), k  # captured == eager, bit for bit
    assert not torch.equal(runs[True]["p"], runs[True]["ema"])
    miss = {}
    for k in ("p", "ema", "loss", "norm"):
        got = runs[True][k].double().cpu()
        err, e32 = _rel(got, h64[k]), _rel(h32[k], h64[k])
        # a row crossing a knot of the spline at another step in f32 than in f64 makes the two host loops part ways (the gradient
        # jumps there): such a draw fails here instead of widening the bound
        assert e32 <= 1e-4, f"{kind}: ill-conditioned draw, the f32 host loop itself misses the f64 one by {e32:.2e} in {k}"
        bound = FACTOR * max(e32, FLOOR)
        print(f"{kind} trajectory {k}: kernel {err:.3e}  host f32 {e32:.3e}  bound {bound:.3e}")
        if not err <= bound:
            miss[k] = (err, bound)
    assert not miss, miss


def test_a_nan_row_skips_the_step():
    m = PC.make_pgm("flow", seed=23)
    obs = {k: v.cuda() for k, v in PC.draw(m, 48, seed=4).items()}
    ts = _step_cls()(m, **HP)
    for _ in range(3):
        ts.step(**obs)
    before = [t.clone() for t in (ts._on.flat_p, ts._ema.flat_p, ts.m, ts.v)]
    bad = {k: v.clone() for k, v in obs.items()}
    bad["brain_volume"][7, 0] = float("nan")
    out = ts.step(**bad)
    torch.cuda.synchronize()
    st = ts.stats()
    assert math.isnan(float(out["loss"])) and st["n_skipped"] == 1 and st["skipped_last"] and st["opt_steps"] == 3
    for a, b in zip(before, (ts._on.flat_p, ts._ema.flat_p, ts.m, ts.v)):
        assert torch.equal(_bits(a), _bits(b))
    ts.step(**obs)
    assert ts.stats()["opt_steps"] == 4 and not ts.stats()["skipped_last"]


@pytest.mark.parametrize("kind", ("flow", "morpho"))
def test_step_from_a_table_equals_step_on_the_rows(kind):
    from causal_gen_amd.pgm_train import default_columns

    m = PC.make_pgm(kind, seed=25)
    cols, ncol = default_columns(m)
    pool = PC.draw(m, 300, seed=6)
    table = torch.zeros(300, ncol + 2)  # (two foreign columns at the end, as a data set's parents table may have)
    for var, c0 in cols.items():
        table[:, c0:c0 + pool[var].shape[1]] = pool[var]
    table = table.cuda()
    g = torch.Generator().manual_seed(7)
    a = _step_cls()(copy.deepcopy(m), columns=cols, ncol=ncol + 2, **HP)
    b = _step_cls()(copy.deepcopy(m), **HP)
    for t in range(4):
        index = torch.randint(0, 300, (70,), generator=g).cuda()
        oa = a.step_from(table, index)
        ob = b.step(**{var: table[index, c0:c0 + pool[var].shape[1]] for var, c0 in cols.items()})
        assert torch.equal(_bits(oa["loss"]), _bits(ob["loss"])) and torch.equal(_bits(oa["grad_norm"]), _bits(ob["grad_norm"])), t
    torch.cuda.synchronize()
    assert len(a._graphs) == 1
    for x, y in ((a._on.flat_p, b._on.flat_p), (a._ema.flat_p, b._ema.flat_p), (a.m, b.m), (a.v, b.v), (a.state, b.state)):
        assert torch.equal(_bits(x), _bits(y))
    # an index outside the table poisons the loss and the step is skipped: nothing is read out of bounds
    index = torch.randint(0, 300, (70,), generator=g).cuda()
    index[3] = 300
    out = a.step_from(table, index)
    assert math.isnan(float(out["loss"])) and a.stats()["n_skipped"] == 1


def test_loss_is_the_loss_of_step_on_the_same_parameters():
    m = PC.make_pgm("chest", seed=27)
    obs = {k: v.cuda() for k, v in PC.draw(m, 48, seed=8).items()}
    ts = _step_cls()(m, **HP)
    for _ in range(3):  # (the third step is a replay)
        want = ts.loss(**obs)
        got = ts.step(**obs)["loss"]
        assert torch.equal(_bits(want), _bits(got))


@pytest.mark.parametrize("kind", PC.KINDS)
def test_state_dict_loads_as_a_reference_checkpoint(kind):
    from causal_gen_amd import dscm
    from causal_gen_amd.cf_eval import CfEvaluator

    m = PC.make_pgm(kind, seed=29)
    obs = {k: v.cuda() for k, v in PC.draw(m, 48, seed=9).items()}
    ts = _step_cls()(m, **HP)
    for _ in range(4):
        ts.step(**obs)
    sd = ts.state_dict()
    assert {"model_state_dict", "ema_model_state_dict", "optimizer_state_dict", "step"} <= set(sd)
    var = next(iter(m.variables))
    do = {var: obs[var].flip(0)}
    for key, src in (("model_state_dict", ts.model), ("ema_model_state_dict", ts.ema_model)):
        fresh = PC.make_pgm(kind, seed=31).cuda()
        ckpt = dict(sd[key])
        ckpt["encoder_s.cnn.0.weight"] = torch.zeros(3)  # a reference checkpoint carries its predictors on the same module
        assert fresh.load_reference_state_dict(ckpt) == ["encoder_s.cnn.0.weight"]
        for mod in (fresh, src):
            if kind == "chest":
                mod.generator = torch.Generator(device="cuda").manual_seed(3)
        want, got = src.counterfactual(obs, do), fresh.counterfactual(obs, do)
        for k in want:
            assert torch.equal(want[k], got[k]), (key, k)
    # a second step object resumes bit for bit
    ts2 = _step_cls()(PC.make_pgm(kind, seed=31), **HP)
    ts2.load_state_dict(sd)
    la, lb = ts.step(**obs)["loss"], ts2.step(**obs)["loss"]
    torch.cuda.synchronize()
    assert torch.equal(_bits(la), _bits(lb)) and ts.it == ts2.it == 5
    for a, b in ((ts._on.flat_p, ts2._on.flat_p), (ts._ema.flat_p, ts2._ema.flat_p), (ts.m, ts2.m), (ts.v, ts2.v), (ts.state, ts2.state)):
        assert torch.equal(_bits(a), _bits(b))
    # the EMA model is the PGM the counterfactual stages take
    args = SimpleNamespace(lmbda_init=1.0, elbo_constraint=2.0, dataset="none")
    model = dscm.DSCM(args, ts.ema_model, None, None)
    assert model.pgm is ts.ema_model and not any(p.requires_grad for p in model.pgm.parameters())
    ev = CfEvaluator(None, ts.ema_model, None, args, specs=[])
    assert ev.pgm is ts.ema_model


def test_a_fit_recovers_the_generating_model():
    """512 rows from a seeded FlowPGM, a freshly initialised one trained on them for 200 full-batch steps at lr 3e-2.  The host
    f32 loop (same optimiser) goes from 9.001 to 4.592 on one CPU and to 4.609 on another, 0.13 .. 0.14 BELOW the generating
    model's own nll on those rows, 4.735 (a maximum-likelihood fit of 512 rows beats the model that drew them); the margin given to
    both, on either side, is 0.2.  The kernel ended at 4.608."""
    MARGIN = 0.2
    truth = PC.make_pgm("flow", seed=33)
    rows = PC.draw(truth, 512, seed=10)
    torch.manual_seed(0)
    from causal_gen_amd.pgm import FlowPGM

    fresh = FlowPGM(SimpleNamespace())
    hp = dict(HP, lr=3e-2, ema_update_after=100)
    with torch.no_grad():
        target = float(PC.to64(truth).nll(PC.cast(rows, torch.float64)))
        start = float(PC.to64(fresh).nll(PC.cast(rows, torch.float64)))
    h32, hm = host_loop(fresh, [rows], 200, torch.float32, hp)
    with torch.no_grad():
        host_final = float(hm.nll(rows))
    ts = _step_cls()(copy.deepcopy(fresh), **hp)
    dev = {k: v.cuda() for k, v in rows.items()}
    first = float(ts.loss(**dev))
    for _ in range(200):
        ts.step(**dev)
    final = float(ts.loss(**dev))
    print(f"fit: generating model {target:.4f}, start {start:.4f} (kernel {first:.4f}), host loop {host_final:.4f}, kernel {final:.4f}")
    assert abs(host_final - target) <= MARGIN, (host_final, target)
    assert final < first and abs(final - target) <= MARGIN, (first, final, target)
