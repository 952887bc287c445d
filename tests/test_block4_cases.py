"""The CPU side of tests/test_gpu_block4_f64.py: a plain-Python mirror of b4_fill and of the launch decision agrees with cgen_block4_plan
(host code) over a sweep of argument records, the sweep reaches exactly the instance keys the case table covers, the table holds the
conditions it is about, the entry points decline what they must, the staged f64 reference of tests/block4_ref.py is torch's conv2d /
autograd of the default Block, the bound passes the 16-bit rounding of the reference and rejects every mutant on every case it applies
to (both 16-bit formats), and the recorded constants -- accumulation, GELU table, flagged share -- are what the CPU measures."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import block4_cases as T
import block4_ref as R


@pytest.fixture(scope="module")
def lib():
    from causal_gen_amd import _lib

    return _lib.load()


ALL = T.CASES + [c for pair in T.PAIRS for c in pair]


# ------------------------------------------------------------------------------------------------- plan, mirror, keys
def test_every_case_plans_to_the_instance_it_names(lib):
    assert len({c.id() for c in ALL}) == len(ALL)
    for c in ALL:
        a = T.args(c)
        ok, key, vals = T.plan(lib, a)
        want = c.key if c.key[0] != "pair" else ("dgrad", c.key[1], 4)
        assert ok == 1 == lib.block4_supported(C.byref(a)) and key == want, (c.id(), ok, key, c.key)
        assert (key, vals) == T.mirror(a), (c.id(), vals)
        assert (vals["ntiles"], vals["tiles_x"], vals["tiles_y"], vals["nch0"]) == (c.ntiles,) + c.tiles + (c.nch0,)
        assert key[1] == c.nb8


def test_the_mirror_agrees_with_the_plan_over_the_sweep_and_the_table_covers_what_it_reaches(lib):
    recs = T.sweep_records()
    assert len(recs) >= 20000
    reached, declined = set(), 0
    for a in recs:
        out = (C.c_int32 * T.PLAN_INTS)(*([-7] * T.PLAN_INTS))
        ok = lib.block4_plan(C.byref(a), out)
        want = T.mirror(a)
        assert ok == lib.block4_supported(C.byref(a)) == int(want is not None), (a.fwd, a.n, a.h, a.w, a.b, a.nseg, a.nout)
        if ok:
            assert (T.key_of(tuple(out)), {k: out[i] for k, i in T.PLAN_FIELDS.items()}) == want
            reached.add(want[0])
        else:
            declined += 1
            assert all(v == -7 for v in out)  # (a declined record leaves out[] alone)
    assert declined > 1000
    # the keys the sweep reaches at the default knobs: what the plan of this work expected, no difference to write down
    assert reached == T.EXPECTED_KEYS == {c.key for c in T.CASES}, (sorted(reached ^ T.EXPECTED_KEYS), sorted(T.EXPECTED_KEYS - {c.key for c in T.CASES}))
    assert len(reached) == 21


def test_pair_plan_names_the_pair_kernel_of_each_class(lib):
    assert [p[0].key for p in T.PAIRS] == [("pair", nb8) for nb8 in T.NB8S]
    for ca, cb in T.PAIRS:
        a, b = T.args(ca), T.args(cb)
        out = (C.c_int32 * T.PLAN_INTS)()
        assert lib.block4_pair_plan(C.byref(a), C.byref(b), out) == lib.block4_pair_supported(C.byref(a), C.byref(b)) == 1
        assert tuple(out[:7]) == (0, ca.key[1], 4, ca.ntiles, ca.ntiles + cb.ntiles, T.lds_bytes(ca.key[1]), cb.ntiles) and not any(out[7:])
        assert (ca.ntiles, cb.ntiles) == (8, 7) and ca.b != cb.b and ca.nb8 == cb.nb8
    # other classes, or a forward record, do not pair
    (a0, _), (a1, _) = T.PAIRS[0], T.PAIRS[1]
    assert lib.block4_pair_plan(C.byref(T.args(a0)), C.byref(T.args(a1)), None) == lib.block4_pair_supported(C.byref(T.args(a0)), C.byref(T.args(a1))) == 0
    f = T.args(T.CASES[0])
    assert lib.block4_pair_plan(C.byref(f), C.byref(f), None) == 0


@pytest.mark.parametrize("name,base,change,gpu", T.DECLINED, ids=[d[0] for d in T.DECLINED])
def test_declined_records_are_refused_by_supported_plan_and_the_mirror(lib, name, base, change, gpu):
    a = T.args(base)
    assert lib.block4_supported(C.byref(a)) == 1 and T.mirror(a) is not None
    change(a)
    out = (C.c_int32 * T.PLAN_INTS)()
    assert lib.block4_supported(C.byref(a)) == 0 and lib.block4_plan(C.byref(a), out) == 0 and T.mirror(a) is None


def test_the_table_holds_the_conditions_it_is_about():
    fwd = [c for c in T.CASES if c.dir == "fwd"]
    dg = [c for c in T.CASES if c.dir == "dgrad"]
    bs = {c.b for c in T.CASES}
    assert bs & {4, 5, 6} and bs >= {8, 12, 20, 24, 32, 48, 60, 64} and bs & {36, 40}
    for d in (fwd, dg):
        assert {c.nb8 for c in d} == set(T.NB8S)
        assert any(c.ntiles <= 16 for c in d) and any(c.ntiles > 1024 and c.ntiles % 8 for c in d)
        assert any(512 <= c.ntiles <= 1024 and c.ntiles % 8 for c in d)
        assert any(c.tiles[0] == 1 for c in d) and any(c.tiles[0] > 1 and c.w % 16 for c in d)
        assert {(c.h, c.w) for c in d} >= {(1, 1), (4, 4), (8, 16), (9, 17)} and {(c.h, c.w) for c in d} & {(7, 9), (13, 33)}
        assert {c.layout for c in d} == {"dense", "chan", "win"}
    assert {c.key[2] for c in fwd if c.ntiles > 1024} == {4} and {c.key[2] for c in fwd if c.ntiles <= 1024} == {8}
    assert all(max(c.segs + [c.co]) <= 16 for c in T.CASES if c.ntiles > 1024)
    assert {len(c.segs) for c in fwd} == {1, 2, 3}
    widths = {s for c in fwd for s in c.segs}
    assert widths >= {8, 16, 32, 40, 12, 6} and any(c.flat(6) and not c.flat(12) for c in fwd)
    nch = {c.nch0 for c in fwd}
    assert nch >= {1, 2, 3} and any(v >= 4 and v % 2 == 0 for v in nch)
    assert {c.co for c in fwd} >= {8, 24, 40, 256}
    assert {(bool(c.res[0]), c.rem) for c in fwd} >= {(False, ""), (True, ""), (False, "o"), (True, "r"), (True, "or")}
    assert any("0" in c.bias for c in fwd) and any(c.bias == "0000" for c in fwd) and any(c.bias == "1111" for c in fwd)
    assert {c.nout for c in dg} == {1, 2, 3}
    assert any(0 < sum(c.res) < c.nout for c in dg) and any(c.nout > 1 and c.res[1] for c in dg)
    assert any(s > 256 for c in dg for s in c.segs) and {c.co for c in dg} >= {8, 24, 160, 224}


# ------------------------------------------------------------------------------------------------- the references are torch's
SMALL = [c for c in ALL if c.n * c.h * c.w <= 1500]


def _gelu16(t, tdt):
    return F.gelu(t).to(tdt).double()


@pytest.mark.parametrize("case", [c for c in SMALL if c.dir == "fwd"], ids=lambda c: c.id())
def test_forward_reference_is_torch_f64(case):
    I = R.make_inputs(case)
    tdt = I.tdt
    bias = [None if b is None else b.double() for b in I.bias]
    x = torch.cat([s.expand(case.n, case.h, case.w, s.shape[3]) for s in I.segs], -1).permute(0, 3, 1, 2)
    chain = R.reference_chain(case, I)
    t = x
    for s in range(4):
        y = F.conv2d(_gelu16(t, tdt), I.Wq[s], bias[s], padding=I.Wq[s].shape[2] // 2)
        if s == 3 and I.res1 is not None:
            y = y + I.res1.permute(0, 3, 1, 2) + (0 if I.res1_rem is None else I.res1_rem.permute(0, 3, 1, 2))
        ref = chain[s] if s < 3 else chain[3][0]
        assert float((ref.ref.permute(0, 3, 1, 2) - y).abs().max()) <= 1e-12, s
        t = y.to(tdt).double()


@pytest.mark.parametrize("case", [c for c in SMALL if c.dir == "dgrad"], ids=lambda c: c.id())
def test_data_gradient_reference_is_torch_autograd(case):
    """Every stage is one conv + GELU of the forward Block differentiated by autograd: y = conv(gelu(u)) with u the stage's aux tensor
    (so that gelu' is taken where the kernel takes it), backward from the stage's incoming gradient."""
    I = R.make_inputs(case)
    tdt = I.tdt
    chain = R.reference_chain(case, I)
    gin = I.g.permute(0, 3, 1, 2)
    for s in range(3):
        u = I.aux[s].permute(0, 3, 1, 2).clone().requires_grad_(True)
        w = I.Wq[3 - s]
        F.conv2d(F.gelu(u), w, padding=w.shape[2] // 2).backward(gin)
        assert float((chain[s].ref.permute(0, 3, 1, 2) - u.grad).abs().max()) <= 1e-12, s
        gin = R.rn16(u.grad, tdt)
    xs = [torch.zeros(case.n, c, case.h, case.w, dtype=torch.float64) for c in case.segs]
    for j, k in enumerate(case.dsegs):
        xs[k] = I.x[j].permute(0, 3, 1, 2).clone()
    xs = [x.requires_grad_(True) for x in xs]
    F.conv2d(F.gelu(torch.cat(xs, 1)), I.Wq[0]).backward(gin)
    for j, k in enumerate(case.dsegs):
        want = xs[k].grad + (0 if I.res[j] is None else I.res[j].permute(0, 3, 1, 2))
        assert float((chain[3][j].ref.permute(0, 3, 1, 2) - want).abs().max()) <= 1e-12, (j, k)


# ------------------------------------------------------------------------------------------------- the bound
_WORST = {}


def _applies(case, m):
    """Must the mutant m apply to the case (at one stage at least)?"""
    fwd = case.dir == "fwd"
    if not R.MUTANTS[m][0 if fwd else 1]:
        return False
    widths = case.segs if fwd else [case.co]
    return {
        "tap": case.h >= 2 and case.w >= 3,
        "halo_gelu_bias": case.bias[0] == "1" or case.bias[1] == "1",
        "bias_last": "1" in case.bias[:3],
        "chunk_hi": any((c - 1) % 32 >= 16 for c in widths),
        "seg_alias": len(case.segs) > 1,
        "res1_last_row": any(case.res),
        "res1_rem": "r" in case.rem,
        "acc_out1": case.nout > 1 and bool(case.res[1]),
    }.get(m, True)


@pytest.mark.parametrize("bf16", [False, True], ids=["binary16", "bfloat16"])
@pytest.mark.parametrize("case", ALL, ids=lambda c: c.id())
def test_the_bound_passes_the_reference_and_rejects_every_mutant(case, bf16):
    full = R.make_inputs(case, bf16)
    I = R.images(case, full, slice(0, 4)) if case.n * case.h * case.w > 4096 else full  # (a mutant that fails on four images fails on the case)
    tdt = I.tdt
    chain = R.reference_chain(case, I)
    prevs = [None] + [R.rn16(chain[s].ref, tdt) for s in range(3)]
    stages = [(s, 0, chain[s]) for s in range(3)] + [(3, j, r) for j, r in enumerate(chain[3])]
    for s, j, ref in stages:
        w, bad = R.worst(R.stored(ref, tdt), ref, tdt)
        assert bad == 0 and w <= 1.0, (s, j, w)
        key = (case.dir, bf16, s)
        _WORST[key] = max(_WORST.get(key, 0.0), w)
        assert I is not full or ref.flag_share <= R.FLAG_SHARE_MAX  # (the condition is on the whole case)
    applied = set()
    for m in R.MUTANTS:
        for s, j, ref in stages:
            mut = R.stage(case, I, s, prevs[s], m, j)
            if mut is None:
                continue
            assert R.worst(R.stored(mut, tdt, m), ref, tdt)[1] > 0, f"stage {s}, output {j}: the bound passes the mutant {m}"
            applied.add(m)
    must = {m for m in R.MUTANTS if _applies(case, m)}
    assert must <= applied, must - applied


def test_remainder_planes_of_the_reference_meet_their_bound():
    case = next(c for c in T.CASES if c.rem == "or")
    I = R.make_inputs(case)
    ref = R.reference_chain(case, I)[3][0]
    hi = R.rn16(ref.ref, I.tdt)
    rem = R.rn16(ref.ref - hi, I.tdt)
    assert bool(R.nearest16(hi, rem, I.tdt).all())
    assert R.worst(hi + rem, ref, I.tdt, half_ulp_of=rem)[1] == 0
    assert R.worst(hi + 3 * rem, ref, I.tdt, half_ulp_of=rem)[1] > 0


def test_the_reference_sits_inside_its_own_bound():
    """(after the parametrised test: the worst err / tol of the 16-bit rounding of the reference -- half an ulp over half an ulp + T)"""
    if _WORST:
        print("reference against its own bound, worst err/tol:", {k: round(v, 4) for k, v in _WORST.items()})
        assert all(0.5 < v <= 1.0 for v in _WORST.values())


# ------------------------------------------------------------------------------------------------- the recorded constants
def test_the_recorded_accumulation_constants_are_what_the_chain_measures():
    got = R.measure_k_acc(T.CASES)
    assert set(got) == set(R.K_ACC)
    for kind, e in got.items():
        assert R.K_MARGIN * e <= R.K_ACC[kind] < R.K_MARGIN * e + 1.0, (kind, e, R.K_ACC[kind])


def test_the_table_mirror_gives_the_recorded_deltas():
    f = b = 0.0
    for tdt in (torch.float16, torch.bfloat16):
        x = R.all_finite16(tdt)
        assert x.numel() == {torch.float16: 63488, torch.bfloat16: 65280}[tdt]
        ef, eb = R.measure_lut(tdt)
        f, b = max(f, ef), max(b, eb)
    assert max(R.K_MARGIN * f, R.TRUNC_FWD) <= R.DELTA_FWD < 1.05 * R.K_MARGIN * f, f
    assert max(R.K_MARGIN * b, R.TRUNC_BWD) <= R.DELTA_BWD < 1.05 * R.K_MARGIN * b, b
    # the mirror is the kernel's arithmetic: 385 entries on the grid i / 32, exact at the grid points up to the f32 rounding of Phi
    tab = R.lut_tables(True)
    assert tab.shape == (385, 3) and float(tab[192, 0]) == 0.5 and float(tab[0, 0]) < 1e-8 and float(tab[384, 0]) == 1.0
    x0 = torch.tensor([-6.0, -1.0, 0.0, 0.5, 6.0, 7.0, -9.0], dtype=torch.float64)
    assert torch.equal(R.lut(x0, tab), tab[[0, 160, 192, 208, 384, 384, 0], 0].double())


def test_every_forward_case_keeps_the_flagged_share_below_the_cap():
    for bf16 in (False, True):
        for c in T.CASES:
            if c.dir == "fwd":
                I = R.make_inputs(c, bf16)
                assert len(I.flag_shares) == 4 and max(I.flag_shares) < R.FLAG_SHARE_MAX, (c.id(), I.flag_shares)
