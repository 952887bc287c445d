"""The CPU side of tests/test_gpu_block3_f64.py: the case table names the instances it means to (cgen_block3_plan is host code), a sweep
of the planner reaches no instance the table leaves out, the f64 references of tests/block_ref.py are torch's conv2d / autograd of the
light Block, the bound rejects every mutant on every case and passes the reference, and the recorded accumulation constants are what the
sequential f32 chain measures."""
import pytest
import torch
import torch.nn.functional as F

import block_cases as T
import block_ref as R


@pytest.fixture(scope="module")
def lib():
    from causal_gen_amd import _lib

    return _lib.load()


def test_every_case_plans_to_the_instance_it_names(lib):
    assert len({c.id() for c in T.CASES}) == len(T.CASES)
    for c in T.CASES:
        ok, key, vals = T.plan(lib, T.args(c))
        assert ok and key == c.key, (c.id(), ok, key, c.key)
        assert ok == (2 if key[0] == "rows" else 1)
        assert {k: vals[k] for k in c.about} == c.about, (c.id(), vals, c.about)


# Instances the dispatch at the end of csrc/block.hip can name but no argument record reaches (read from b3_fill / b3_plan): none -- every
# instantiation of blk3_kernel, blk3s_kernel and blk3r_kernel behind cgen_block3 is reached.  What looks missing is not instantiated:
#   tile SM = 1 with NB >= 3 or NPG = 4   b3_plan: wb_persist wants nb <= 2 and one or two pairs
#   tile TH = 12 with NB = 4 or NPG < 4   b3_plan: twelve rows only for npg == 4, sm == 0, nb <= 3
#   tile REM with PRE = 0 or SM = 1       b3_fill: remainder planes are forward only; b3_plan: they clear the streaming mode
#   rows RES = 1 with PRE = 0             b3_fill: r_res_tile wants pre_act
#   rows PROJ forward with RES != 0       b3_fill: the down Block's forward has no other residual
#   rows NR = 2                           compiled under -DB3R_TRIAL only
UNREACHABLE = set()


def test_the_sweep_reaches_exactly_the_instances_the_table_covers(lib):
    recs = T.sweep_records()
    assert len(recs) >= 3000
    reached = set()
    for c in recs:
        a = T.args(c)
        ok, key, _ = T.plan(lib, a)
        assert ok == lib.block3_supported(a), (c.dir, c.n, c.h, c.w, c.segs, c.b, c.co, c.res1, c.rem, c.a16, c.down)
        if ok:
            reached.add(key)
    covered = {c.key for c in T.CASES}
    assert reached | UNREACHABLE == covered | UNREACHABLE, (sorted(reached - covered), sorted(covered - reached))
    assert len(reached) == 87


def test_the_table_holds_the_conditions_it_is_about():
    tile = [c for c in T.CASES if c.family() == "tile"]
    small = [c for c in T.CASES if c.family() == "small"]
    rows = [c for c in T.CASES if c.family() == "rows"]
    for d in ("fwd", "dgrad"):
        t = [c for c in tile if c.dir == d]
        assert {c.about["ns"] for c in t} == {2, 3}
        assert any(c.about["ntiles"] > c.about["grid"] for c in t)
        assert any(c.about["ntiles"] <= 256 for c in t) and any(c.about["ntiles"] > 256 and c.about["ns"] == 3 for c in t)
        assert {c.b for c in t} == {8, 16, 24, 32} and {len(c.segs) for c in t} == {1, 2, 3}
        assert any(c.h % 8 for c in t) and any(c.w % 16 for c in t) and any(c.co % 32 for c in t)
        assert any(s % 8 for c in t for s in c.segs) and any(s % 32 and not s % 8 for c in t for s in c.segs)
        s = [c for c in small if c.dir == d]
        assert {min(c.about["s_rows"], 4) for c in s} == {2, 3, 4}  # (a strip of ONE row is only ever the last, short one: 64 / w - 2 >= 2)
        assert any(c.h % c.about["s_rows"] == 1 for c in s) and any(c.about["s_strips"] == 1 for c in s)
        assert {c.about["s_nmb"] for c in s} == {1, 2} and {c.b for c in s} >= {40, 48, 64} and all(c.n <= 4 for c in s)
        r = [c for c in rows if c.dir == d]
        assert any(c.about["r_sy"] == 1 for c in r) and any(c.about["r_sy"] > 1 and c.h % 4 for c in r) and any(c.w % 32 for c in r)
    assert any(c.nout == 2 for c in tile) and any(c.rg == [1, 0, 1] for c in tile)
    assert {c.res1 for c in rows if c.dir == "fwd"} == {None, "alias", "own"} and {c.about["r_res_tile"] for c in rows} == {0, 1}
    assert {c.bias for c in tile} == {"both", "a", "o", "none"} and {c.layout for c in T.CASES} == {"dense", "chan", "win"}
    assert any(c.a16 is False and c.w >= 48 and c.h >= 16 and c.segs == [32] for c in tile)
    # ragged then full in one persistent workgroup: tile 2 of 172 x 20 x 16 has four rows, tile 2 + 512 has eight
    c = next(c for c in tile if c.name == "persist-sm-ragged-then-full")
    assert (c.about["grid"], c.about["ntiles"]) == (512, 516) and 2 % 3 == 2 and (2 + 512) % 3 == 1 and c.h == 20


# ------------------------------------------------------------------------------------------------- the references are torch's
def _torch_block(case, I):
    """The light Block in torch f64 with the quantised weights: (x leaves, t, y before any residual)."""
    xs = [x.permute(0, 3, 1, 2).expand(x.shape[0], x.shape[3], case.h, case.w).clone().requires_grad_(True) for x in I.segs]
    t = F.conv2d(F.relu(torch.cat(xs, 1)), I.w1q, None if I.bias_a is None else I.bias_a.double(), padding=1)
    return xs, t


SMALL = [c for c in T.CASES if c.n * c.h * c.w <= 4000]


@pytest.mark.parametrize("case", [c for c in SMALL if c.dir == "fwd"], ids=lambda c: c.id())
def test_forward_reference_is_torch_f64(case):
    I = R.make_inputs(case)
    with torch.no_grad():
        xs, t = _torch_block(case, I)
        assert float((R.stage1(case, I).ref.permute(0, 3, 1, 2) - t).abs().max()) <= 1e-12
        mid = R.rn16(t, I.tdt)
        y = F.conv2d(F.relu(mid), I.w2q, None if I.bias_o is None else I.bias_o.double(), padding=1)
        if case.down:
            y = F.avg_pool2d(y + F.conv2d(xs[0], I.wpq, None if I.bias_p is None else I.bias_p.double()), 2)
        if I.res1 is not None:
            y = y + I.res1.permute(0, 3, 1, 2) + (0 if I.res1_rem is None else I.res1_rem.permute(0, 3, 1, 2))
        (ref,) = R.stage2(case, I, mid.permute(0, 2, 3, 1))
        assert float((ref.ref.permute(0, 3, 1, 2) - y).abs().max()) <= 1e-12


@pytest.mark.parametrize("case", [c for c in SMALL if c.dir == "dgrad"], ids=lambda c: c.id())
def test_data_gradient_reference_is_torch_autograd(case):
    """The forward Block on fresh inputs whose differentiable segments ARE the case's aux tensors and whose bottleneck is its mid_aux."""
    I = R.make_inputs(case)
    J = R.make_inputs(T.Case(case.name, "fwd", case.n, case.h, case.w, case.segs, case.b, case.co, bias="none"))
    for j, k in enumerate(case.dsegs):
        J.segs[k] = I.x[j]
    J.w1q, J.w2q = I.w1q, I.w2q
    xs, t = _torch_block(case, J)
    # relu'(t) is taken from the case's own mid_aux (directed values): a straight-through product in place of torch's threshold
    tm = I.t.permute(0, 3, 1, 2)
    y = F.conv2d(t * (tm > 0), I.w2q, padding=1)
    if case.down:
        y = y + F.conv2d(xs[0], I.wpq)
    y.backward(I.g.permute(0, 3, 1, 2))
    s1 = R.stage1(case, I)
    gt = F.conv_transpose2d(I.g.permute(0, 3, 1, 2), I.w2q, padding=1) * (tm > 0)
    assert float((s1.ref.permute(0, 3, 1, 2) - gt).abs().max()) <= 1e-12
    refs = R.stage2(case, I, s1.ref)
    for j, k in enumerate(case.dsegs):
        want = xs[k].grad + (0 if I.res[j] is None else I.res[j].permute(0, 3, 1, 2))
        assert float((refs[j].ref.permute(0, 3, 1, 2) - want).abs().max()) <= 1e-12, (j, k)


# ------------------------------------------------------------------------------------------------- the bound
_WORST = {}


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id())
def test_the_bound_passes_the_reference_and_rejects_every_mutant(case):
    full = R.make_inputs(case)
    big = case.n * case.h * case.w > 8192
    I = R.images(case, full, slice(0, 2)) if big else full  # (a mutant that fails on two images fails on the case)
    tdt = I.tdt
    r1 = R.stage1(case, I)
    mid = R.rn16(r1.ref, tdt)
    r2 = R.stage2(case, I, mid)
    w1, bad1 = R.worst(mid, r1, tdt)
    assert bad1 == 0 and w1 <= 1.0
    for ref in r2:
        w2, bad2 = R.worst(R.stored(ref, tdt), ref, tdt)
        assert bad2 == 0 and w2 <= 1.0
        _WORST[case.family()] = max(_WORST.get(case.family(), 0.0), w1, w2)
    applied = []
    for m in R.STAGE1_MUTANTS:
        mut = R.stage1(case, I, m)
        if mut is not None:
            assert R.worst(R.stored(mut, tdt, m), r1, tdt)[1] > 0, f"stage 1: the bound passes the mutant {m}"
            applied.append(m)
    for m in R.STAGE2_MUTANTS:
        if m == "stale_mid":
            continue
        muts = R.stage2(case, I, mid, m)
        if muts is not None:
            for j, (mut, ref) in enumerate(zip(muts, r2)):
                assert R.worst(R.stored(mut, tdt, m), ref, tdt)[1] > 0, f"stage 2, output {j}: the bound passes the mutant {m}"
            applied.append(m)
    if case.family() == "tile" and case.about["ntiles"] > case.about["grid"]:
        fmid = R.rn16(R.stage1(case, full).ref, tdt)
        muts = R.stage2(case, full, fmid, "stale_mid")
        n1 = muts[0].image
        refs = R.stage2(case, R.images(case, full, slice(n1, n1 + 1)), fmid[n1:n1 + 1])
        for mut, ref in zip(muts, refs):
            assert R.worst(R.stored(mut, tdt), ref, tdt)[1] > 0, "stage 2: the bound passes the mutant stale_mid"
        applied.append("stale_mid")
    # what has to apply to every case of a direction
    must = {"a_tap", "b_tap", "wrap_input", "swap_pair", "rtz"} | ({"relu_neg_as_one", "relu_zero_as_one"} if case.dir == "dgrad" else set())
    if case.dir == "fwd" and case.bias in ("both", "a"):
        must |= {"bias_a_last", "halo_bias"}
    if case.res1:
        must.add("res1_last_row")
    if (sum(case.segs) if case.dir == "fwd" else case.co) > 32:
        must.add("kdrop")
    assert must <= set(applied), must - set(applied)


def test_the_reference_sits_inside_its_own_bound():
    """(after the parametrised test: the worst err / tol of the 16-bit rounding of the reference, per family -- half an ulp over
    half an ulp + T, so just below 1)"""
    if _WORST:
        print("reference against its own bound, worst err/tol:", {k: round(v, 4) for k, v in _WORST.items()})
        assert all(0.5 < v <= 1.0 for v in _WORST.values())


def test_the_recorded_accumulation_constants_are_what_the_chain_measures():
    got = R.measure_k_acc(T.CASES)
    for fam, e in got.items():
        assert R.K_MARGIN * e <= R.K_ACC[fam] < R.K_MARGIN * e + 1.0, (fam, e, R.K_ACC[fam])
    assert set(got) == set(R.K_ACC)
