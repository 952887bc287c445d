"""The CPU side of tests/test_gpu_wgrad_f64.py: the plain-Python mirror of cgen_conv2d_wgrad's dispatch (tests/wgrad_cases.py) agrees with
cgen_conv2d_wgrad_plan_record of the built library (host code: no GPU) on every case and on a seeded sweep around the thresholds; the
table reaches every instance and boundary it claims; the f64 reference (tests/wgrad_ref.py) agrees with autograd; the tolerance tells
every mutant from the reference; the flagged share of the 16-bit GELU operands is within FLAG_SHARE_MAX.

The accumulation constants of the tolerance, measured by `python tests/wgrad_ref.py` (worst error of one sequential f32 fmaf chain over
the pixel axis, in units of 2^-24 A, over the inputs of every case; IEEE binary16 build) and what K_MARGIN = 4 makes of them:

  family     measured   K_ACC
  f32-gen    2.671      11
  h16-gen    4.173      17
  h16-tile   4.109      17

test_k_acc_is_what_the_chain_measures re-measures a subset."""
import ctypes as C
import math
import random

import pytest
import torch
import torch.nn.functional as F

import wgrad_cases as T
import wgrad_ref as R

BASE = 1 << 20  # a 256-byte aligned stand-in address: the plan queries dereference nothing


def lib_record(lib, q, monkeypatch):
    from causal_gen_amd import _lib

    if q["generic"]:
        monkeypatch.setenv("CGEN_WGRAD_GENERIC", "1")
    else:
        monkeypatch.delenv("CGEN_WGRAD_GENERIC", raising=False)
    a = _lib.WgradArgs()
    a.dtype = _lib.F32 if q["dt"] == "f32" else _lib.F16
    a.n, a.h, a.w, a.ks, a.nseg, a.act = q["n"], q["h"], q["w"], q["ks"], len(q["seg"]), q["act"]
    for s, v in enumerate(q["seg"]):
        a.seg[s] = _lib.View(BASE + v["p"], v["sn"], v["sh"], v["sw"], v["c"], v["cpad"])
    v = q["gout"]
    a.gout = _lib.View(BASE + v["p"], v["sn"], v["sh"], v["sw"], v["c"], v["cpad"])
    a.partial_w, a.partial_b = BASE, (BASE if q["bias"] else None)
    rec = (C.c_int32 * T.REC_INTS)(*([-1] * T.REC_INTS))
    kind = C.c_int32(-1)
    ns = lib.conv2d_wgrad_plan_record(C.byref(a), rec)
    assert ns == rec[1] == lib.conv2d_wgrad_plan(C.byref(a), C.byref(kind)) and kind.value == rec[0]
    return list(rec)


@pytest.fixture(scope="module")
def lib():
    from causal_gen_amd import _lib

    return _lib.load()


PLANS = {c.id(): T.plan(T.problem(c)) for c in T.CASES}


def test_ids_are_unique_and_cases_are_small():
    assert len({c.id() for c in T.CASES}) == len(T.CASES)
    for c in T.CASES:
        assert c.macs() < 5 * 10 ** 8 < T.MAC_CAP, c.id()
        assert c.unscale == 1.0 or math.frexp(c.unscale)[0] == 0.5  # a power of two
    # below 10^7 multiply-adds wherever the kernel under test allows it: the tiled instances start at 256 and 520 channels on both sides
    assert all(c.macs() < 10 ** 7 for c in T.CASES if max(sum(c.segs), c.co) < 256)


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id())
def test_case_lands_on_its_instance_and_mirror_equals_library(lib, case, monkeypatch):
    q = T.problem(case)
    assert T.tag(PLANS[case.id()]) == case.want
    assert T.record(q) == lib_record(lib, q, monkeypatch)


def _sweep(count, seed):
    rnd = random.Random(seed)
    wide = list(range(248, 273, 4)) + list(range(512, 529, 4)) + [250, 255, 257, 515, 521] + list(range(560, 705, 8)) + [1016, 1024, 1032]
    narrow = [1, 3, 5, 8, 12, 15, 16, 17, 24, 31, 32, 33, 40, 63, 64, 65, 96, 100, 130]
    out = []
    while len(out) < count:
        dt = rnd.choice(["h16", "h16", "h16", "f32"])
        ks = rnd.choice([1, 3, 3, 5, 7])
        big = rnd.random() < 0.5 and ks in (1, 3)
        nseg = rnd.choice([1, 1, 2, 3])
        segs = [rnd.choice(wide if big and s == 0 else narrow) for s in range(nseg)]
        co = rnd.choice(wide if big and rnd.random() < 0.8 else narrow)
        n, h, w = rnd.randint(1, 5), rnd.choice([1, 2, 6, 7, 8, 9, 15, 16, 17, 33]), rnd.choice([1, 2, 6, 8, 11, 12, 15, 16, 17, 24, 33])
        if rnd.random() < 0.3:  # P around 256 (one or two splits of the generic kernel)
            n, h, w = 1, 16, rnd.choice([15, 16, 17])
        style = rnd.choice(["pad8", "pad8", "pad8", "tight", "odd", "unpadded"])
        mk = {"pad8": T.pad8, "tight": T.tight, "odd": lambda c: T.V(1), "unpadded": lambda c: T.V(8, 0, 0)}[style]
        views = tuple(mk(c) for c in segs)
        if nseg > 1 and rnd.random() < 0.3:
            views = views[:1] + (T.V(8, 0, T._pad(segs[1], 8), True),) + views[2:]
        out.append(T.Case(dt, n, h, w, tuple(segs), co, ks, rnd.choice([0, 1, 2]), views, mk(co), bias=rnd.random() < 0.7,
                          generic=rnd.random() < 0.1))
    return out


# What serves kind 1 at the default knobs, as (NCF, NJW, KS): cwin, LDS bytes.  <4, 6, 3> and <6, 4, 1> take the square wide layers (3x3 from
# 256 -> 256, 1x1 from 520 -> 520); wgrad2_geometry's co-block search hands some 3x3 input widths (296, 328, 360, 520 -> 264 ...) to <2, 16, 3>
# and <2, 12, 3>; 1x1 from 568 -> 584 on (640 -> 640, 1024 -> 1024) is <8, 3, 1>'s and some of it (584 -> 680 ...) <4, 6, 1>'s.  Held over
# the seeded sweep below and over every pair of 8-granular widths of one dense segment up to 1104 channels, plus 1536, 2048 and 4096.
TILED_INSTANCES = {(4, 6, 3): (32, 45056), (6, 4, 1): (112, 65536), (2, 16, 3): (112, 67584), (2, 12, 3): (80, 57344), (8, 3, 1): (64, 73728),
                   (4, 6, 1): (160, 73728)}


def test_tiled_instances_over_every_dense_width_up_to_1104(lib, monkeypatch):
    """Every (ci, co) of multiples of 8 up to 1104, and 1536 / 2048 / 4096, one dense 8-padded 16-bit segment, 1x1 and 3x3 (the image
    size enters the split only): the mirror's tiled instances are exactly TILED_INSTANCES, all single-buffered; the library agrees on
    every 97th pair and on the first pair of each instance."""
    ch = list(range(8, 1105, 8)) + [1536, 2048, 4096]
    seen, k = {}, 0
    for ks in (1, 3):
        for ci in ch:
            for co in ch:
                q = T.problem(T.Case("h16", 2, 12, 12, (ci,), co, ks, views=(T.pad8(ci),), gv=T.pad8(co)))
                p = T.plan(q)
                k += 1
                first = p["kind"] == 1 and (p["ncf"], p["njw"], p["ks"]) not in seen
                if p["kind"] == 1:
                    assert p["dbuf"] == 0
                    seen.setdefault((p["ncf"], p["njw"], p["ks"]), set()).add((p["cwin"], p["lds"]))
                if first or k % 97 == 0:
                    assert T.record(q) == lib_record(lib, q, monkeypatch), (ks, ci, co)
    assert seen == {k: {v} for k, v in TILED_INSTANCES.items()}, seen


def test_mirror_equals_library_on_a_sweep_and_every_tiled_instance_has_a_case(lib, monkeypatch):
    kinds, tiled = {}, set()
    for c in _sweep(4000, 20261021):
        q = T.problem(c)
        m = T.record(q)
        assert m == lib_record(lib, q, monkeypatch), c
        kinds[m[0]] = kinds.get(m[0], 0) + 1
        if m[0] == 1:
            tiled.add((m[2], m[3], m[4]))
    assert all(kinds.get(k, 0) >= 100 for k in (0, 1, 2, 3)), kinds
    covered = {(p["ncf"], p["njw"], p["ks"]) for p in PLANS.values() if p["kind"] == 1}
    assert tiled == set(TILED_INSTANCES) == covered, f"tiled instances without a case: {sorted(tiled - covered)}"


def test_thresholds_of_the_tiled_kernel(lib, monkeypatch):
    """At the default knobs, on dense 8-padded 16-bit views: 3x3 with both sides >= 256 and 1x1 with both sides >= 520 are the tiled
    kernel's (the streaming kernel finds no tile ring for them), one step below on either side the streaming kernel's."""
    for ks, lo in ((3, 256), (1, 520)):
        for n, h, w in ((2, 6, 6), (1, 33, 17), (4, 1, 1)):
            for ci, co, want in ((lo, lo, 1), (lo + 8, lo, 1), (lo, lo + 8, 1), (lo - 8, lo, None), (lo, lo - 8, None)):
                q = T.problem(T.Case("h16", n, h, w, (ci,), co, ks))
                rec = lib_record(lib, q, monkeypatch)
                assert rec == T.record(q)
                assert (rec[0] == 1) if want else (rec[0] in (2, 3)), (ks, n, h, w, ci, co, rec[:2])


def test_the_table_reaches_what_it_claims():
    by = lambda f: [c for c in T.CASES if f(c, PLANS[c.id()])]  # noqa: E731
    for dt in ("f32", "h16"):
        gen = by(lambda c, p: p["kind"] == 0 and c.dt == dt)
        assert {PLANS[c.id()]["ntc"] for c in gen} == {1, 2, 4}
        assert {PLANS[c.id()]["n_tapgroups"] for c in gen} == {1, 3, 6}
        assert {PLANS[c.id()]["gout_vec"] for c in gen} == {0, 1}
        assert {PLANS[c.id()]["seg_vec"] & 1 for c in gen} == {0, 1}
        assert any(len(c.segs) > 1 for c in gen) and any(c.v(s).bcast for c in gen for s in range(len(c.segs)))
        assert {c.act for c in gen} == {0, 1, 2}
        assert dt == "h16" or {c.bias for c in gen} == {True, False}  # (the ResNet's calls pass no bias partial)
        assert any(c.h * c.w == 1 and c.ks == 3 for c in gen) and any(c.h < c.ks and c.ks == 7 for c in gen)
        # a ragged last split whose last K-step is ragged too
        rag = [PLANS[c.id()] | dict(P=c.n * c.h * c.w) for c in gen if PLANS[c.id()]["nsplit"] >= 2]
        assert any(p["P"] % p["pix_per_split"] and (p["P"] % p["pix_per_split"]) % T.WG_PK for p in rag)
        # a bias whose Co spans two co tiles
        assert any(c.bias and c.co > PLANS[c.id()]["ntc"] * 16 for c in gen)
    p = PLANS[next(c for c in T.CASES if c.dt == "f32" and (c.n, c.h, c.w) == (3, 10, 11)).id()]
    assert (p["nsplit"], p["pix_per_split"]) == (2, 192) and 330 - 192 == 138 and 138 % 64 == 10
    assert any(c.generic and PLANS[c.id()]["kind"] == 0 and c.dt == "h16" for c in T.CASES)
    assert any(PLANS[c.id()]["n_cichunks"] == 144 for c in T.CASES) and any(c.v(0).step == 2 for c in T.CASES)
    for inst in sorted(TILED_INSTANCES):
        tl = by(lambda c, p: p["kind"] == 1 and (p["ncf"], p["njw"], p["ks"]) == inst)
        assert {c.act for c in tl} == {0, 1, 2}
        ctot8 = lambda c: sum(T._pad(s, 8) for s in c.segs)  # noqa: E731
        assert any(ctot8(c) % PLANS[c.id()]["cwin"] for c in tl), "no ragged last window"
        assert any(c.co % (inst[0] * 16) for c in tl), "no ragged last co block"
        assert all(PLANS[c.id()]["dbuf"] == 0 for c in tl)
    tl = by(lambda c, p: p["kind"] == 1)
    assert any(len(c.segs) > 1 and c.v(1).bcast for c in tl)
    assert {(p["ncf"], p["njw"], p["ks"], p["cwin"], p["lds"]) for p in map(lambda c: PLANS[c.id()], tl)} == {k + v for k, v in TILED_INSTANCES.items()}
    p = PLANS[next(c for c in tl if (c.n, c.h, c.w) == (1, 17, 9)).id()]
    assert p["nsplit"] == 2 and p["ntiles"] - p["tps"] == 1, "two splits, the last of one tile"


_SMALL = [c for c in T.CASES if c.macs() < 5 * 10 ** 7]


@pytest.mark.parametrize("case", _SMALL, ids=lambda c: c.id())
def test_reference_is_autograd_in_f64(case):
    I = R.make_inputs(case)
    plan = PLANS[case.id()]
    ref = R.reference(case, I, plan)
    a = R.activated(case, I, plan["kind"])[0].permute(0, 3, 1, 2)
    w = torch.zeros((case.co, sum(case.segs), case.ks, case.ks), dtype=torch.float64, requires_grad=True)
    b = torch.zeros((case.co,), dtype=torch.float64, requires_grad=True)
    (F.conv2d(a, w, b, padding=case.ks // 2) * I.g.permute(0, 3, 1, 2)).sum().backward()
    want_w = w.grad * case.unscale + (I.prev_w if case.accumulate else 0)
    assert float((ref.w - want_w).abs().max()) <= 1e-12 * float(ref.A_w.max())
    if case.bias:
        want_b = b.grad * case.unscale + (I.prev_b if case.accumulate else 0)
        assert float((ref.b - want_b).abs().max()) <= 1e-12 * float(ref.A_b.max())
    else:
        assert ref.b is None
    assert bool((ref.tol_w > 0).all()) or case.act != T.NONE  # (a ReLU column may be all zeros: then the sum is exactly zero)


@pytest.fixture(scope="module")
def mutant_table():
    """{case id: {mutant: told apart?}} over the mutants that apply to the case, computed once (a few seconds) and shared."""
    table = {}
    for case in T.CASES:
        I = R.make_inputs(case)
        plan = PLANS[case.id()]
        ref = R.reference(case, I, plan)
        row = table[case.id()] = {}
        for m in R.MUTANTS:
            mut = R.reference(case, I, plan, m)
            if mut is not None and not R.identical(ref, mut):
                row[m] = R.told_apart(ref, mut)
    return table


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id())
def test_every_applicable_mutant_is_told_from_the_reference(case, mutant_table):
    for m, told in mutant_table[case.id()].items():
        assert told, f"{m} passes the tolerance of {case.id()}"


def test_every_mutant_applies_in_each_kind_it_is_meaningful_for(mutant_table):
    for m in R.MUTANTS:
        kinds = {PLANS[cid]["kind"] for cid, row in mutant_table.items() if m in row}
        assert kinds == set(R.MUTANT_KINDS[m]), (m, kinds)


def test_flagged_share_of_the_rounded_gelu_operands():
    n = 0
    for bf16 in (False, True):
        for c in T.CASES:
            if c.act == T.GELU and PLANS[c.id()]["kind"] == 1:
                I = R.make_inputs(c, bf16)
                assert R.activated(c, I, 1)[3] <= R.FLAG_SHARE_MAX, (c.id(), bf16, I.salt)
                n += 1
    assert n >= 6


def test_k_acc_is_what_the_chain_measures():
    """K_ACC = ceil(K_MARGIN x the worst chain error over the table).  The full measurement is `python tests/wgrad_ref.py` (every case,
    2^22 multiply-adds each); its figures are the literals below.  Here a subset (every fourth case, 2^20) must stay at or below them."""
    worst = R.measure_k_acc(T.CASES[::4], budget=1 << 20)
    assert set(worst) == set(R.K_ACC)
    recorded = {"f32-gen": 2.671, "h16-gen": 4.173, "h16-tile": 4.109}
    for fam, e in worst.items():
        assert 0.5 < e <= recorded[fam] + 1e-3, (fam, e)
        assert R.K_ACC[fam] == math.ceil(R.K_MARGIN * recorded[fam])
