"""Counterfactual parents on the MI355X (causal_gen_amd.pgm_cf over csrc/pgm_cf.hip) against ``pgm.counterfactual``,
``ukbb_preprocess`` and ``_abduct`` of the f64 CPU copy of the same PGM, with the f32 inputs cast to f64.

Bounds follow tests/test_gpu_pgm_train.py's rule; nothing is fixed in advance.  For each compared column the test measures e32, the
deviation of the SAME host code run in f32 on the CPU from the f64 oracle, relative to max(1, |oracle|), and holds the kernel to
4 * max(e32, 2^-24).  What must be exact is asserted on the bits: intervened columns are the ``do`` rows', untouched and foreign
columns the observation's, the empty mask returns the table and pa == cf_pa.  A Gumbel-max class is compared on every row whose
top-two margin in the oracle is at least 1e-4 (at most 2 % of the rows may fall below it).

Measured on the MI355X over the 30 shape cases (every case prints its figures; LABNOTES 20).  Host f32 against f64, non-zero
columns: touched continuous cf 9.8e-9 .. 4.3e-7 (median 1.7e-7), eps 2.4e-9 .. 4.7e-6, pa 2.2e-7 .. 5.4e-6, cf_pa up to 5.6e-6 (the
log-standardised UKBB volumes); bounds therefore 2.4e-7 (the floor) .. 2.2e-5.  The kernel: cf <= 2.1e-7 (median 7.2e-8), eps <= 8.1e-8,
pa <= 5.6e-8, cf_pa <= 1.7e-6, round trip <= 1.2e-7; at most 0.29 of its bound anywhere.  Clamp rows: e32 0.88 by design, the kernel
against the f32 host run 4.5e-8 .. 2.4e-7 on the values and 1.8e-5 on the thickness noise.  ChestPGM finding under do(age): classes
equal on every row, no row below the margin (smallest 8.0e-4 / 6.2e-4 for the two posteriors).
"""
import copy
import functools
from types import SimpleNamespace

import pytest
import torch

import pgm_cases as PC

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -24
FACTOR = 4.0
MARGIN = 1e-4

ARGS = {"flow": SimpleNamespace(parents_x=["mri_seq", "brain_volume", "ventricle_volume", "age", "sex"], dataset="ukbb192"),
        "morpho": SimpleNamespace(parents_x=["thickness", "intensity", "digit"], dataset="morphomnist"),
        "colour": SimpleNamespace(parents_x=["digit", "colour"], dataset="cmnist"),
        "chest": SimpleNamespace(parents_x=["age", "race", "sex", "finding"], dataset="mimic")}

# tag: (kind, hidden widths or None for the PGM's own, rows); 64 rows = one workgroup; edge rows from 65 up
CASES = {}
for _k in PC.KINDS:
    for _b in (1, 2, 63, 64, 65, 129):
        CASES[f"{_k}_b{_b}"] = (_k, None, _b)
for _k in ("flow", "morpho"):
    for _w in ([8, 16], [64], [64, 64, 64]):
        CASES[f"{_k}_w{'x'.join(map(str, _w))}"] = (_k, _w, 65)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _mod():
    from causal_gen_amd import pgm_cf

    return pgm_cf


def _layout(m, extra=2):
    from causal_gen_amd.pgm_train import default_columns

    cols, ncol = default_columns(m)
    width = {mech.var: (mech.module.shape[-1] if mech.kind == "categorical" else 1) for mech in m.mechanisms()}
    return cols, ncol + extra, width


def _table(m, obs, seed=0):
    """[B, ncol + 2] f32 table of `obs` in the default layout with two foreign columns at the end (as a data set's table may have)."""
    cols, ncol, width = _layout(m)
    B = next(iter(obs.values())).shape[0]
    t = torch.randn(B, ncol, generator=torch.Generator().manual_seed(500 + seed))
    for var, c0 in cols.items():
        t[:, c0:c0 + width[var]] = obs[var]
    return t


def _interventions(m, kind):
    out = [[v] for v in m.variables] + [[], list(m.variables)]
    if kind == "flow":
        out.append(["sex", "age"])
    return out


def _finding_oracle(mm, obs, cf_age, u, exact):
    """(class, top-two margin) of `finding` from the posterior noise of the observed class with the uniforms `u`."""
    from causal_gen_amd import pgm as P

    post = P.gumbel_max_abduct_exact if exact else P.gumbel_max_abduct
    noise = post(obs["finding"], mm.finding_logits(obs["age"]), u=u.to(obs["age"].dtype))
    score = noise + mm.finding_logits(cf_age)
    top = score.topk(2, -1).values
    return score.argmax(-1, keepdim=True).to(obs["age"].dtype), (top[:, 0] - top[:, 1])


def host_eval(m, kind, obs, do_vars, perm, dtype, u=None, exact=False):
    """cf {var: [B, k]}, eps {var: [B, 1]}, pa / cf_pa [B, ctx] and the finding margin, by the host code on the CPU in `dtype`."""
    from causal_gen_amd import dscm

    mm = copy.deepcopy(m).cpu().to(dtype)
    o = {k: v.cpu().to(dtype) for k, v in obs.items()}
    do = {k: o[k][perm] for k in do_vars}
    margin = None
    with torch.no_grad():
        cf = mm.counterfactual(o, do)
        if kind == "chest" and "finding" not in do and "age" in do:
            cf["finding"], margin = _finding_oracle(mm, o, cf["age"], u, exact)
        eps = {k: v for k, v in mm._abduct(o).items() if k != "finding"}
    args = ARGS[kind]

    def pre(pa):
        pa = dscm.ukbb_preprocess(pa) if "ukbb" in args.dataset else pa
        return torch.cat([pa[k] for k in args.parents_x], 1)

    return dict(cf={k: v.double() for k, v in cf.items()}, eps={k: v.double() for k, v in eps.items()}, pa=pre(o).double(),
                cf_pa=pre(cf).double(), margin=margin)


def _dev(got, ref):
    """per column: max over rows of |got - ref| / max(1, |ref|)"""
    return ((got.double() - ref).abs() / ref.abs().clamp_min(1.0)).amax(0)


def _pa_columns(m, kind):
    """{variable: slice of the parents row}"""
    _, _, width = _layout(m)
    out, o = {}, 0
    for k in ARGS[kind].parents_x:
        out[k] = slice(o, o + width[k])
        o += width[k]
    return out


class Runner:
    """One PgmCounterfactual and the device copies of a batch."""

    def __init__(self, m, kind, obs, perm, exact=None):
        cols, ncol, self.width = _layout(m)
        self.cols = cols
        self.cf = _mod().PgmCounterfactual(copy.deepcopy(m), ARGS[kind], columns=cols, ncol=ncol, exact_gumbel=exact)
        self.table = _table(m, obs).cuda()
        self.perm = perm.cuda()
        self.B = self.table.shape[0]

    def run(self, do_vars, uniforms=None):
        cf, pa, cf_pa = self.cf.run(self.table, None, self.table, self.perm, do_vars=do_vars, uniforms=None if uniforms is None else uniforms.cuda())
        out = dict(table=cf.clone(), pa=pa.clone(), cf_pa=cf_pa.clone(), eps=self.cf.noise(self.B).clone())
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in out.items()}

    def col(self, t, var):
        return t[:, self.cols[var]:self.cols[var] + self.width[var]]


@functools.lru_cache(maxsize=None)
def _case(tag):
    kind, widths, B = CASES[tag]
    m = PC.make_pgm(kind, seed=0, widths=widths)
    obs = PC.draw(m, B, seed=B)
    if B >= 65:
        obs = PC.edge_rows(m, obs, kind)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(7))
    u = torch.rand(B, 2, generator=torch.Generator().manual_seed(11))
    return m, kind, obs, perm, u


def _hold(tag, rows):
    """rows: (name, kernel deviation, e32)"""
    miss = {}
    for name, err, e32 in rows:
        bound = FACTOR * max(e32, FLOOR)
        print(f"{tag} {name}: kernel {err:.3e}  host f32 {e32:.3e}  bound {bound:.3e}")
        if not err <= bound:
            miss[name] = (err, bound)
    assert not miss, (tag, miss)


def _compare(tag, m, kind, got, r64, r32, run, do_vars, obs_table, perm):
    """The bounded comparisons of one (case, intervention) and the bit-exact ones."""
    cf_mod = _mod()
    touched = cf_mod.touched(m, do_vars)
    rows = []
    name = "do(" + ",".join(do_vars) + ")"
    keep = None
    if r64["margin"] is not None:
        keep = r64["margin"] >= MARGIN
        left = 1.0 - keep.double().mean().item()
        print(f"{tag} {name}: finding rows below the margin {left:.4f}, smallest margin {r64['margin'].min().item():.3e}, "
              f"flipped {(r64['cf']['finding'] != r32['cf']['finding']).double().mean().item():.4f} host f32 vs f64")
        assert left <= 0.02, left
    for var in m.variables:
        g = run.col(got["table"], var)
        if var in do_vars:  # the do rows' bits
            assert torch.equal(_bits(g), _bits(run.col(obs_table[perm], var))), (tag, name, var)
        elif var not in touched:  # the observation's bits
            assert torch.equal(_bits(g), _bits(run.col(obs_table, var))), (tag, name, var)
        elif var == "finding":
            assert torch.equal(g.double()[keep], r64["cf"]["finding"][keep]), (tag, name, "finding classes on the rows above the margin")
        else:
            rows.append((f"{name} cf {var}", _dev(g, r64["cf"][var]).max().item(), _dev(r32["cf"][var], r64["cf"][var]).max().item()))
    assert torch.equal(_bits(got["table"][:, -2:]), _bits(obs_table[:, -2:])), (tag, name, "foreign columns")
    for var, sl in _pa_columns(m, kind).items():
        sel = keep if (var == "finding" and keep is not None and var in touched and var not in do_vars) else slice(None)
        for which in ("pa", "cf_pa"):
            rows.append((f"{name} {which} {var}", _dev(got[which][sel, sl], r64[which][sel, sl]).max().item(),
                         _dev(r32[which][sel, sl], r64[which][sel, sl]).max().item()))
    for i, mech in enumerate(m.mechanisms()):
        e = got["eps"][:, i:i + 1]
        if mech.var in r64["eps"]:
            rows.append((f"{name} eps {mech.var}", _dev(e, r64["eps"][mech.var]).max().item(),
                         _dev(r32["eps"][mech.var], r64["eps"][mech.var]).max().item()))
        else:
            assert bool((e == 0).all()), (tag, name, mech.var, "roots and Gumbel-max report no noise")
    if not do_vars:
        assert torch.equal(_bits(got["table"]), _bits(obs_table)), (tag, "the empty mask returns the observation table")
        assert torch.equal(_bits(got["pa"]), _bits(got["cf_pa"])), (tag, "pa == cf_pa under the empty mask")
    _hold(tag, rows)


@pytest.mark.parametrize("tag", sorted(CASES))
def test_counterfactuals_match_the_f64_host(tag):
    """Every single variable, the empty mask, all variables (and {sex, age} for flow), do rows = a seeded permutation of the batch.
    Measured (LABNOTES 20): e32 of the touched continuous variables 9.8e-9 .. 4.3e-7, the kernel <= 2.1e-7 and at most 0.29 of a
    bound; every line printed is kernel deviation, host-f32 deviation and bound."""
    m, kind, obs, perm, u = _case(tag)
    run = Runner(m, kind, obs, perm)
    obs_table = run.table.cpu()
    for do_vars in _interventions(m, kind):
        got = run.run(do_vars, u if kind == "chest" else None)
        r64 = host_eval(m, kind, obs, do_vars, perm, torch.float64, u)
        r32 = host_eval(m, kind, obs, do_vars, perm, torch.float32, u)
        _compare(tag, m, kind, got, r64, r32, run, do_vars, obs_table, perm)


def test_morpho_rows_at_the_clamp_of_the_normalisation():
    """thickness and intensity at +-1 and +-(1 - 1e-7) saturate the dtype's clamp: f32 and f64 differ there by design, so these
    rows are additionally held to the f32 host run itself at 1e-3 (test_gpu_pgm_train.py gives the reason)."""
    m = PC.make_pgm("morpho", seed=13)
    obs = PC.clamp_rows(m)
    perm = torch.randperm(8, generator=torch.Generator().manual_seed(7))
    run = Runner(m, "morpho", obs, perm)
    obs_table = run.table.cpu()
    for do_vars in (["thickness"], ["intensity"], ["digit"], []):
        got = run.run(do_vars)
        for k in ("table", "pa", "cf_pa", "eps"):
            assert bool(torch.isfinite(got[k]).all()), (do_vars, k)
        r64 = host_eval(m, "morpho", obs, do_vars, perm, torch.float64)
        r32 = host_eval(m, "morpho", obs, do_vars, perm, torch.float32)
        _compare("morpho_clamp", m, "morpho", got, r64, r32, run, do_vars, obs_table, perm)
        vs32 = {"thickness": _dev(run.col(got["table"], "thickness"), r32["cf"]["thickness"]).max().item(),
                "intensity": _dev(run.col(got["table"], "intensity"), r32["cf"]["intensity"]).max().item(),
                "cf_pa": _dev(got["cf_pa"], r32["cf_pa"]).max().item(), "pa": _dev(got["pa"], r32["pa"]).max().item(),
                "eps thickness": _dev(got["eps"][:, 1:2], r32["eps"]["thickness"]).max().item(),
                "eps intensity": _dev(got["eps"][:, 2:3], r32["eps"]["intensity"]).max().item()}
        print("morpho_clamp", do_vars, "against the f32 host run:", {k: f"{v:.2e}" for k, v in vs32.items()})
        assert max(vs32.values()) <= 1e-3, (do_vars, vs32)


@pytest.mark.parametrize("exact", (0, 1))
@pytest.mark.parametrize("B", (65, 129, 1024))
def test_chest_finding_under_do_age_matches_the_oracle_classes(B, exact):
    """Uniforms (seed 11) shared with the f64 oracle through ``u=``; the classes match on every row whose top-two margin in the
    oracle is at least 1e-4, and at most 2 % of the rows may be left out.  Oracle-only figures (CPU, f64; the MI355X run printed
    the same): exact_gumbel = 0 leaves out no row (smallest margins 4.0e-2, 9.0e-3, 8.0e-4 at 65, 129, 1024 rows) and flips 6.2 %,
    1.6 %, 5.4 % of the findings under do(age), so a kernel that copied the observation would fail; exact_gumbel = 1 leaves out no row
    either (9.4e-3, 1.2e-2, 6.2e-4) and flips 0, 0 and 0.2 %.  The kernel's classes equalled the oracle's on every row."""
    m = PC.make_pgm("chest", seed=0)
    obs = PC.draw(m, B, seed=B)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(7))
    u = torch.rand(B, 2, generator=torch.Generator().manual_seed(11))
    run = Runner(m, "chest", obs, perm, exact=bool(exact))
    got = run.run(["age"], u)
    r64 = host_eval(m, "chest", obs, ["age"], perm, torch.float64, u, exact=bool(exact))
    keep = r64["margin"] >= MARGIN
    want = r64["cf"]["finding"]
    flipped = (want != obs["finding"].double()).double().mean().item()
    left = 1.0 - keep.double().mean().item()
    print(f"chest B={B} exact={exact}: left out {left:.4f}, smallest margin {r64['margin'].min().item():.3e}, oracle flips {flipped:.4f}")
    assert left <= 0.02, left
    g = run.col(got["table"], "finding").double()
    assert torch.equal(g[keep], want[keep])
    assert bool(((g == 0) | (g == 1)).all())
    if not exact:
        assert flipped > 0.0  # (the test can fail: the counterfactual finding is not the observed one everywhere)


@pytest.mark.parametrize("kind", ("flow", "morpho", "chest"))
def test_gather_equals_the_run_on_the_gathered_rows(kind):
    m = PC.make_pgm(kind, seed=25)
    cols, ncol, _ = _layout(m)
    table = _table(m, PC.draw(m, 300, seed=6)).cuda()
    g = torch.Generator().manual_seed(7)
    index, do_index = torch.randint(0, 300, (70,), generator=g).cuda(), torch.randint(0, 300, (70,), generator=g).cuda()
    u = torch.rand(70, 2, generator=g).cuda() if kind == "chest" else None
    do_vars = ["age"] if kind != "morpho" else ["thickness"]
    a = _mod().PgmCounterfactual(copy.deepcopy(m), ARGS[kind], columns=cols, ncol=ncol)
    b = _mod().PgmCounterfactual(copy.deepcopy(m), ARGS[kind], columns=cols, ncol=ncol)
    keys = ("cf", "pa", "cf_pa")
    ga = dict(zip(keys, [t.clone() for t in a.run(table, index, table, do_index, do_vars=do_vars, uniforms=u)]), eps=a.noise(70).clone())
    gb = dict(zip(keys, [t.clone() for t in b.run(table[index].contiguous(), None, table[do_index].contiguous(), None, do_vars=do_vars, uniforms=u)]),
              eps=b.noise(70).clone())
    for k in ga:
        assert torch.equal(_bits(ga[k]), _bits(gb[k])), k
    # an index outside either table: that row is NaN in every output, the other rows keep their bits; nothing is read out of bounds
    for which, bad in (("index", 300), ("index", -1), ("do_index", 300)):
        i2, d2 = index.clone(), do_index.clone()
        (i2 if which == "index" else d2)[3] = bad
        out = dict(zip(keys, a.run(table, i2, table, d2, do_vars=do_vars, uniforms=u)), eps=a.noise(70))
        rest = torch.arange(70, device="cuda") != 3
        for k in out:
            assert bool(torch.isnan(out[k][3]).all()), (which, bad, k)
            assert torch.equal(_bits(out[k][rest]), _bits(ga[k][rest])), (which, bad, k)
    # without an intervention the do index is not looked at
    out = a.run(table, index, table, torch.full_like(do_index, 10 ** 9), do_vars=[], uniforms=u)[0]
    assert torch.equal(_bits(out), _bits(table[index]))


@pytest.mark.parametrize("tag", ("flow_b129", "morpho_w64x64x64", "chest_b65"))
def test_reruns_are_bit_identical(tag):
    m, kind, obs, perm, u = _case(tag)
    do_vars = {"flow": ["sex"], "morpho": ["thickness"], "chest": ["age"]}[kind]
    runs = [Runner(m, kind, obs, perm).run(do_vars, u if kind == "chest" else None) for _ in range(2)]
    for k in runs[0]:
        assert torch.equal(_bits(runs[0][k]), _bits(runs[1][k])), k


@pytest.mark.parametrize("kind", ("flow", "morpho", "chest"))
def test_captured_run_follows_index_do_index_and_device_mask(kind):
    """``run`` captured once with a device mask; each replay after changing the CONTENTS of the index, the do index and the mask
    word equals the eager call with the same inputs, bit for bit."""
    m = PC.make_pgm(kind, seed=27)
    cols, ncol, _ = _layout(m)
    table = _table(m, PC.draw(m, 200, seed=8)).cuda()
    g = torch.Generator().manual_seed(9)
    B = 70
    draw = lambda: torch.randint(0, 200, (B,), generator=g).cuda()
    index, do_index, mask = draw(), draw(), torch.zeros(1, dtype=torch.int32, device="cuda")
    u = torch.rand(B, 2, generator=g).cuda() if kind == "chest" else None
    cap = _mod().PgmCounterfactual(copy.deepcopy(m), ARGS[kind], columns=cols, ncol=ncol)
    eag = _mod().PgmCounterfactual(copy.deepcopy(m), ARGS[kind], columns=cols, ncol=ncol)
    cap.run(table, index, table, do_index, do_mask_dev=mask, uniforms=u)  # eager first call
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        outs = cap.run(table, index, table, do_index, do_mask_dev=mask, uniforms=u)
    names = [mech.var for mech in m.mechanisms()]
    plans = [[], [names[1]], [names[-1]], names, [names[0], names[-1]]]
    for do_vars in plans:
        index.copy_(draw())
        do_index.copy_(draw())
        mask.fill_(eag.mask_of(do_vars) | (1 << 20))  # (a bit above n is ignored in the device word)
        graph.replay()
        want = eag.run(table, index, table, do_index, do_vars=do_vars, uniforms=u)
        torch.cuda.synchronize()
        for a, b in zip(outs, want):
            assert torch.equal(_bits(a), _bits(b)), do_vars
        assert torch.equal(_bits(cap.noise(B)), _bits(eag.noise(B))), do_vars
    with pytest.raises(ValueError, match="not both"):
        cap.run(table, index, table, do_index, do_vars=["age"], do_mask_dev=mask)


@pytest.mark.parametrize("kind,var", (("flow", "sex"), ("flow", "age"), ("flow", "brain_volume"), ("morpho", "thickness")))
def test_intervening_back_returns_the_original_parents(kind, var):
    """CfEvaluator.reversibility's parents: do(var = another row's value), then do(var = the original value) on the result.  The
    f64 host returns the observation; the kernel is held to 4 * max(e32, 2^-24) with e32 the f32 host round trip's deviation."""
    m = PC.make_pgm(kind, seed=29)
    B = 129
    obs = PC.draw(m, B, seed=10)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(7))
    run = Runner(m, kind, obs, perm)
    there = run.cf.run(run.table, None, run.table, run.perm, do_vars=[var])[0].clone()
    cf, pa, cf_pa = run.cf.run(there, None, run.table, None, do_vars=[var])
    torch.cuda.synchronize()
    cf, cf_pa = cf.cpu(), cf_pa.cpu()

    def host(dtype):
        mm = copy.deepcopy(m).to(dtype)
        o = PC.cast(obs, dtype)
        with torch.no_grad():
            mid = mm.counterfactual(o, {var: o[var][perm]})
            return mm.counterfactual(mid, {var: o[var]})

    h64, h32 = host(torch.float64), host(torch.float32)
    rows = []
    for k in m.variables:
        assert (h64[k] - obs[k].double()).abs().max().item() <= 1e-9, k  # the oracle's round trip is the observation
        rows.append((f"round trip do({var}) {k}", _dev(run.col(cf, k), h64[k]).max().item(), _dev(h32[k].double(), h64[k]).max().item()))
    _hold(f"{kind}_roundtrip", rows)
    assert torch.equal(_bits(run.col(cf, var)), _bits(run.col(run.table.cpu(), var)))


# ----------------------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def morpho():
    from causal_gen_amd import pgm, predictor as P, vae
    from causal_gen_amd.hps import setup_hparams
    from oracle import fullsize_recipe as FR
    from predictor_ref import randomise

    hp = setup_hparams("morphomnist", cond_prior=False)
    hp.dataset = "morphomnist"
    hp.lmbda_init, hp.elbo_constraint = 1.0, 2.0
    torch.manual_seed(7)
    m = vae.HVAE(hp)
    m.apply(FR.init_bias)
    FR.perturb(m)
    m.compute_dtype = "f32"
    m = m.cuda().eval()
    g = torch.Generator().manual_seed(3)
    scm = pgm.MorphoMNISTPGM(SimpleNamespace(widths=[8, 8]))
    with torch.no_grad():
        for p in scm.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.5)
    scm = scm.cuda()
    pred = P.MorphoMNISTPredictor(SimpleNamespace(input_channels=1, input_res=32, std_fixed=0.0))
    randomise(pred, g)
    pred = pred.cuda()
    B = 4
    pa = scm.sample(B, torch.Generator().manual_seed(5))
    x = ((torch.randint(0, 256, (B, 1, 32, 32), generator=g).float() - 127.5) / 127.5).cuda()
    return hp, m, scm, pred, pa, x


def _rng_state(vae):
    eng = vae.engine()
    eng.rng_ptr()
    return eng.rng.clone()


def _hold_parents(tag, scm, pa, do, got):
    cpu = {k: v.cpu() for k, v in pa.items()}
    cdo = {k: v.cpu() for k, v in do.items()}
    outs = {}
    for dtype in (torch.float64, torch.float32):
        mm = copy.deepcopy(scm).cpu().to(dtype)
        with torch.no_grad():
            outs[dtype] = mm.counterfactual(PC.cast(cpu, dtype), PC.cast(cdo, dtype))
    rows = [(f"{tag} {k}", _dev(got[k].cpu(), outs[torch.float64][k]).max().item(),
             _dev(outs[torch.float32][k].double(), outs[torch.float64][k]).max().item()) for k in pa]
    _hold(tag, rows)


def test_dscm_forward_and_effectiveness_with_the_device_pgm(morpho):
    """DSCM.forward under no_grad and CfEvaluator.effectiveness with DevicePGM(pgm) against the host pgm, the HVAE's device RNG
    put back before both runs: parents within the bound above, counterfactual pixels within the project's 1e-3."""
    from causal_gen_amd import cf_eval, dscm

    hp, m, scm, pred, pa, x = morpho
    dev_pgm = _mod().DevicePGM(copy.deepcopy(scm), hp)
    assert dev_pgm.variables == scm.variables and len(dev_pgm.mechanisms()) == 3
    with pytest.raises(ValueError, match="num_particles = 2"):
        dev_pgm.counterfactual(pa, {}, num_particles=2)
    do = {"thickness": pa["thickness"].roll(1, 0)}
    obs = dict(pa, x=x)
    outs = {}
    rng = _rng_state(m)
    for name, p in (("host", copy.deepcopy(scm)), ("device", dev_pgm)):
        model = dscm.DSCM(hp, p, pred, m)
        assert not any(q.requires_grad for q in p.parameters())
        m.engine().rng.copy_(rng)
        with torch.no_grad():
            outs[name] = model(obs, do)
    cfs_h, cfs_d = outs["host"]["cfs"], outs["device"]["cfs"]
    assert float((cfs_h["x"] - cfs_d["x"]).abs().max()) <= 1e-3
    assert float((outs["host"]["elbo"] - outs["device"]["elbo"]).abs()) <= 1e-3 * float(outs["host"]["elbo"].abs())
    _hold_parents("dscm do(thickness)", scm, pa, do, cfs_d)
    assert torch.equal(_bits(cfs_d["thickness"]), _bits(do["thickness"])) and torch.equal(_bits(cfs_d["digit"]), _bits(pa["digit"]))
    assert not torch.equal(cfs_d["intensity"], pa["intensity"])
    # the compact parents of the same call are what vae_preprocess makes of the dict
    want = dscm.vae_preprocess(hp, {k: v.clone() for k, v in cfs_d.items() if k != "x"})[:, :, 0, 0]
    assert torch.equal(_bits(dev_pgm.last_parents[1]), _bits(want))
    eps = dev_pgm.infer_exogeneous(pa)
    host_eps = PC.to64(scm).infer_exogeneous(PC.cast({k: v.cpu() for k, v in pa.items()}, torch.float64))
    assert set(eps) == set(host_eps) == {"thickness_base", "intensity_base"}
    for k in eps:
        assert _dev(eps[k].cpu(), host_eps[k]).max().item() <= 1e-5, k

    dos = {"do(thickness)": do, "do(intensity)": {"intensity": -0.5 * pa["intensity"]}, "do(digit)": {"digit": pa["digit"].roll(1, 0)}, "null": {}}
    imgs = {}
    for name, p in (("host", copy.deepcopy(scm)), ("device", dev_pgm)):
        ev = cf_eval.CfEvaluator(m, p, pred, hp, capacity=64, min_max={"thickness": (0.5, 7.5), "intensity": (60.0, 255.0)})
        m.engine().rng.copy_(rng)
        imgs[name] = ev.effectiveness(obs, dos, return_images=True)
        res = ev.results()["effectiveness"]
        assert res["null"]["n"]["digit"] == x.shape[0]
    for k in dos:
        assert float((imgs["host"][k] - imgs["device"][k]).abs().max()) <= 1e-3, k
    null = dev_pgm.counterfactual(pa, {})
    assert all(torch.equal(_bits(null[k]), _bits(pa[k])) for k in pa)  # the null intervention's parents are the observation's bits
    for k, d in dos.items():
        _hold_parents("effectiveness " + k, scm, pa, d, dev_pgm.counterfactual(pa, d))
