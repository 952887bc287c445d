"""The case table of tests/conv_cases.py, its dispatch mirror and the references of tests/conv_ref.py, checked without a GPU: the table
reaches every arm, instance and boundary cgen_conv2d's dispatch has at the default knobs; the mirror's helpers give the hand-worked values
of conv_shared.h; the references agree with torch autograd and with a recorded fixture; the accumulation term of the tolerance holds
against the sequential-chain emulation; and the tolerance tells every applicable mutant of the reference from the reference.

Accumulation term (conv_ref.K_ACC), measured by `python tests/conv_ref.py` on the inputs of every case of the table -- every output of a
case of up to 2^22 multiply-adds, a drawn sample of the pixels of a larger one -- as the worst |chain - exact| / (2^-24 A) of one k-ordered
f32 fmaf chain, per arm family, then times 4 and rounded up:
    f32-gen 3.607 -> 15    f32-tile 4.047 -> 17    h16-gen 4.495 -> 18    h16-tile 4.202 -> 17
    h16-px  4.697 -> 19    h16-ws   3.938 -> 16    h16-smlp 4.862 -> 20
(test_recorded_k_acc_holds re-measures on a subset.)"""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import conv_cases as T
import conv_ref as R
from conftest import ROOT, load_golden
from gpu_views import assert_bounded

CASES = T.CASES
PLANS = {c.id(): T.plan(c) for c in CASES}


def _of(arm, **kw):
    return [c for c in CASES if PLANS[c.id()]["arm"] == arm and all(getattr(c, k) == v for k, v in kw.items())]


def _pl(c):
    return PLANS[c.id()]


# --------------------------------------------------------------------------------------------------------------- the table
def test_ids_unique_caps_and_intent():
    ids = [c.id() for c in CASES]
    assert len(set(ids)) == len(ids)
    for c in CASES:
        assert c.macs() < T.MAC_CAP, c.id()
        assert c.want and T.plan_tag(c).startswith(c.want), (c.id(), c.want)  # the shape landed where it was written for
        assert c.dir == "fwd" or (c.dt != "f32s" and not c.res2 and not c.bias)
        assert c.force in T.FORCE_ENV
        for role in ("out", "res1"):  # (cgen_conv2d wants remainder-plane offsets in multiples of 16 bytes)
            assert T.rem_offset(c, role) % 16 == 0 or not (c.out_rem or c.res1_rem)
        assert not (c.out_rem or c.res1_rem) or c.dt == "h16"


def test_every_arm_and_instance_is_reached():
    for dir in ("fwd", "dgrad"):
        for dt in ("f32", "h16"):
            assert {_pl(c)["ntc"] for c in _of("gen", dir="fwd", dt=dt)} == {1, 2, 4}
            assert _of("gen", dir=dir, dt=dt)
        assert {(_pl(c)["ntc"]) for c in _of("tile", dir="fwd", dt="f32")} == {1, 2, 4}
        assert any(_pl(c)["windows"] >= 2 for c in _of("tile", dir=dir, dt="f32"))
        assert _of("tile", dir=dir, dt="h16") and any(_pl(c)["rem"] for c in _of("tile", dir=dir, dt="h16"))
        for arm in ("px", "ws", "smlp"):
            assert _of(arm, dir=dir, dt="h16")
    assert {_pl(c)["ntc"] for c in _of("tile", dt="h16")} == {1, 2, 4}
    assert any(_pl(c)["windows"] >= 2 for c in _of("tile", dt="h16"))
    sp = _of("tile", dt="f32s")
    assert len(sp) >= 2 and all(_pl(c)["split"] for c in sp) and {1, 2} <= {_pl(c)["windows"] for c in sp}
    assert {_pl(c)["ntc"] for c in sp} == {1, 2, 4} and {_pl(c)["ntc"] for c in _of("tile", dt="h16") if _pl(c)["rem"]} == {1, 2, 4}
    assert any(_pl(c)["rem"] and T.parent_shape(c, "out")[2] > c.co for c in _of("px"))  # remainder planes with zero padding to write
    # conv_px: (NP, ONESEG, REM, KS) instances and the pixels per piece
    px = _of("px")
    assert {(_pl(c)["np"], _pl(c)["oneseg"], _pl(c)["rem"], c.ks) for c in px} >= {
        (1, True, False, 1), (1, True, False, 3), (1, False, False, 3), (1, True, True, 3), (1, False, True, 1), (2, True, False, 1)}
    assert {_pl(c)["ppp"] for c in px} >= {21, 12, 9, 7, 2, 1}
    assert {_pl(c)["nks"] for c in px} >= {1, 3, 7, 12, 14, 16}
    assert {c.co for c in _of("px", dir="fwd")} >= {8, 32, 40, 64}
    # conv_ws: every bucket that has an instance, both NTC, both segment forms
    ws = _of("ws")
    assert {_pl(c)["bucket"] for c in ws} == set(T.WS_INSTANCES)
    assert {_pl(c)["bucket"] for c in ws if c.force is None} == {5, 6, 8, 10, 12, 16}
    assert {_pl(c)["nkw"] for c in ws} >= {3, 4, 5, 6, 7, 9, 11, 13, 16}
    assert {(_pl(c)["ntc"], _pl(c)["oneseg"]) for c in ws} == {(1, True), (1, False), (2, True), (2, False)}
    assert any(_pl(c)["nk"] % 4 and _pl(c)["nkw"] < _pl(c)["bucket"] for c in ws)  # padding K-steps in the last bucket
    # conv_smallp
    sm = _of("smlp")
    assert {_pl(c)["nks"] for c in sm} >= {1, 3, 4, 5, 16, 17, 60} and {_pl(c)["oneseg"] for c in sm} == {True, False}
    assert {c.co for c in _of("smlp", dir="fwd")} >= {8, 24, 32, 40}
    assert any(c.out_rem and c.res1_rem for c in sm) and any(c.out_rem and not c.res1_rem for c in sm)
    # the data gradient: every dact on every arm, with and without the accumulate, a segment at a non-zero offset
    for arm, dts in (("gen", ("f32", "h16")), ("tile", ("f32", "h16")), ("px", ("h16",)), ("ws", ("h16",)), ("smlp", ("h16",))):
        for dt in dts:
            d = _of(arm, dir="dgrad", dt=dt)
            assert {c.act for c in d} == {T.NONE, T.RELU, T.GELU}, (arm, dt)
            assert {c.res1 for c in d} == {True, False} and any(c.seg_off > 0 for c in d), (arm, dt)


def test_boundaries_have_a_case_on_each_side():
    P = lambda c: c.n * c.h * c.w  # noqa: E731
    for dt in ("f32", "h16"):
        g = _of("gen", dt=dt, dir="fwd")
        assert {P(c) for c in g} >= {127, 128, 129}  # CONV_PT
        assert {c.co for c in g} >= {16, 17, 32, 33, 64, 65}
        assert {c.ks for c in g} == {1, 3, 5, 7}
        assert {c.ks for c in g if c.h == 1 and c.w == 1} == {3, 7}
        assert {len(c.segs) for c in g} == {1, 2, 3, 4} and any(1 in c.segs for c in g)
        assert any(not T.dma_clean(T.view(c, "s0"), c.esz) and c.force is None for c in g)  # ragged, no cpad
        assert any(c.L() % 32 for c in g) and any(not _pl(c)["epi_vec"] for c in g) and any(c.force == "generic" and P(c) > 500 for c in g)
    assert any(c.h < 5 for c in _of("gen", dt="f32") if c.force is None) and any(c.w < 5 for c in _of("gen", dt="f32") if c.force is None)
    t32 = _of("tile", dt="f32", dir="fwd")
    assert {(c.h, c.w) for c in t32} >= {(5, 5), (8, 16), (9, 17), (16, 17), (17, 16)}
    assert {(_pl(c)["ntiles"], c.co > 32, _pl(c)["ntc"]) for c in t32} >= {(191, False, 1), (192, False, 2), (511, True, 2), (512, True, 4), (191, True, 1)}
    assert {c.ks for c in t32} == {1, 3}
    ks = {_pl(c)["k"] for c in t32}  # K around multiples of KSTEP = 16
    assert {8, 16, 24, 72, 144} <= ks
    t16 = _of("tile", dt="h16", dir="fwd")
    assert any(c.force is None and c.co % 8 and P(c) > 6000 for c in t16)
    assert any(c.force is None and _pl(c)["rem"] and math.ceil(c.ks ** 2 * sum(c.segs) / 32) > 16 for c in t16)
    assert any(c.force is None and math.ceil(c.ks ** 2 * sum(c.segs) / 32) > 64 and P(c) > 19000 for c in t16)
    assert any(c.force == "no_px_no_ws" for c in t16)
    # conv_px: 16 K-steps are in, 17 are out; Co % 8 == 4 is in with cpad on every operand and out without; 150 KiB of LDS
    px = _of("px", dir="fwd")
    assert any(_pl(c)["nks"] == 16 for c in px) and any(c.ks == 1 and sum(c.segs) == 544 and _pl(c)["arm"] != "px" for c in CASES)
    assert any(c.co == 12 for c in px) and any(c.co == 12 and c.ks == 3 and P(c) > 6000 and c.dt == "h16" for c in _of("tile"))
    assert any(sum(c.segs) == 256 for c in px) and any(c.ks == 1 and sum(c.segs) == 480 for c in _of("tile", dt="h16"))
    assert {(_pl(c)["np"], c.w) for c in px if c.co == 128} == {(2, 128), (2, 120), (1, 112)}  # 256 tiles x 2 parts = CGEN_PX_MINWG
    assert any((c.h, c.w) == (77, 83) for c in px) and any(P(c) == 6001 for c in px)
    # conv_ws: nkw on both sides of 2 * grid_y; the LDS limit; a ragged image
    ws = _of("ws", dir="fwd")
    assert any(_pl(c)["grid_y"] == 3 and _pl(c)["nkw"] == 6 for c in ws)
    assert any(c.co == 96 and c.segs == (64,) and c.ks == 3 for c in _of("tile", dt="h16"))  # nkw 5 < 6
    assert any(c.force == "no_px" and c.segs == (288,) for c in _of("tile", dt="h16"))  # 128 KiB
    assert any((c.h, c.w) == (77, 83) for c in ws)
    # conv_smallp: the pixel limits, the long-K limit, by side, the centre tap
    sm = _of("smlp", dir="fwd")
    assert {P(c) for c in sm} >= {31, 32, 33, 6000, 19000}
    assert any(P(c) == 19000 and c.segs == (1888,) for c in _of("tile")) and any(P(c) > 19000 and c.segs == (1920,) for c in _of("tile"))
    assert any(min(c.h, c.w) < 5 and P(c) > 6000 for c in sm) and any(c.h == 1 and c.w == 1 and c.ks == 3 for c in sm)


def test_mirror_helpers_on_hand_worked_values():
    v = dict(p=16, sn=8 * 48, sh=8 * 6, sw=8, c=8, cpad=0)
    assert T.vec16_ok(v, 2) and T.vec16_ok(None, 2) and not T.vec16_ok(dict(v, p=8), 2) and not T.vec16_ok(dict(v, sw=12, sh=72, sn=576), 2)
    assert T.vec16_ok(dict(v, sw=4, sh=24, sn=192), 4) and not T.vec16_ok(dict(v, sw=4, sh=24, sn=192), 2)
    assert T.dma_clean(v, 2) and not T.dma_clean(dict(v, c=5), 2) and T.dma_clean(dict(v, c=5, cpad=8), 2) and T.dma_clean(dict(v, c=4), 4)
    assert not T.dma_clean(dict(v, sh=1 << 24), 2) and not T.dma_clean(dict(v, sw=1 << 18), 2) and T.dma_clean(dict(v, sw=(1 << 18) - 8), 2)
    # fits_i32: (n sn + h sh + w sw + c) * 2 < 2^31
    assert T.fits_i32(None, 1, 1, 1) and T.fits_i32(dict(v, sn=(1 << 30) - 8 * 7 - 9), 1, 1, 1) and not T.fits_i32(dict(v, sn=(1 << 30) - 8 * 7 - 8), 1, 1, 1)
    # lds_stride: + 8 elements, then an odd number of 16-byte slots
    assert [T.lds_stride(wd, 2) for wd in (32, 64, 256, 512)] == [40, 72, 264, 520]
    assert [T.lds_stride(wd, 4) for wd in (8, 16, 72)] == [20, 28, 84]
    # mk_pixtile(width, 2, 10, 18): groups per pixel (odd), pixels per 1-KiB piece, pieces per row
    assert [tuple(T.mk_pixtile(wd, 2, 10, 18)[k] for k in ("gpr", "ppp", "ppr", "bytes")) for wd in (8, 24, 40, 56, 224, 264, 504, 512)] == [
        (3, 21, 1, 10240), (5, 12, 2, 20480), (7, 9, 2, 20480), (9, 7, 3, 30720), (29, 2, 9, 92160), (35, 1, 18, 184320), (65, 0, 0, 0), (65, 0, 0, 0)]
    assert T.mk_pixtile(256, 2, 8, 16)["bytes"] == 128 * 1024
    # LDS formulas: conv_px (weights of np pairs + the halo tile), conv_tile (weight slab + halo tile, in whole KiB)
    assert T.px_lds(1, 8, T.mk_pixtile(256, 2, 8, 16)) == 17 * 1024 + 128 * 1024
    assert T.px_lds(2, 3, T.mk_pixtile(8, 2, 10, 18)) == 13 * 1024 + 10 * 1024  # ldw 104 -> 13 groups x 64 rows / 64
    assert T.tile_lds(8, 9, 16, 4, 16, 180) == (6 + 15) * 1024  # kp 80 -> ldw 92: 23 groups x 16 rows = 368; ldc 20: 5 groups x 180 pixels = 900
    assert T.tile_lds(64, 9, 16, 4, 16, 180) > T.TILE_BUDGET >= T.tile_lds(40, 9, 16, 4, 16, 180)


def test_mirror_matches_the_host_code():
    """The constants the mirror copies, and the arm names the hook can return; a change in conv.hip must be carried over.  (The decisions
    themselves are held by tests/test_gpu_conv_f64.py: every case must be served by the arm the mirror predicts.)"""
    src = open(os.path.join(ROOT, "causal-gen_amd", "csrc", "conv.hip")).read()
    shared = open(os.path.join(ROOT, "causal-gen_amd", "csrc", "conv_shared.h")).read()

    def env_default(name):
        return int(re.search(r'env_int\("%s",\s*(\d+)\)' % name, src).group(1))

    def define(text, name):
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))

    assert (env_default("CGEN_SMALLP_MAXP"), env_default("CGEN_SMALLP_MAXP_LONGK"), env_default("CGEN_SMALLP_LONGK")) == (
        T.SMALLP_MAXP, T.SMALLP_MAXP_LONGK, T.SMALLP_LONGK)
    assert (env_default("CGEN_PX_LDS") * 1024, env_default("CGEN_PX_MAXNP"), env_default("CGEN_PX_MINWG")) == (T.PX_LDS_BUDGET, T.PX_MAX_NP, T.PX_MIN_WGS)
    assert env_default("CGEN_WS_MAXLDS") * 1024 == T.WS_MAXLDS and env_default("CGEN_PX_MODE") == 2
    assert (define(src, "CONV_PT"), define(src, "PX_MAXKS"), define(shared, "TILE_H"), define(shared, "TILE_W")) == (T.CONV_PT, T.PX_MAXKS, T.TILE_H, T.TILE_W)
    assert tuple(int(v) for v in re.search(r"buckets\[\]\s*=\s*\{([^}]*)\}", src).group(1).split(",")) == T.WS_BUCKETS
    assert tuple(int(v) for v in re.findall(r"WS_CASE\((\d+)\)", src)) == T.WS_INSTANCES
    assert set(re.findall(r'conv_trace\(\w+(?:\.p)?, "(\w+)"\)', src)) == {"gen", "tile", "px", "ws", "smlp", "smlp2"}
    for name in T.ALL_FORCE_ENV[:3]:
        assert 'getenv("%s")' % name in src  # (read on every call: monkeypatch reaches them)


# --------------------------------------------------------------------------------------------------------------- the references
def _small(dir, dt, act, **kw):
    return T.Case(dir, dt, 2, 5, 6, (3, 4), 5, 3, act=act, **kw)


@pytest.mark.parametrize("act", (T.NONE, T.RELU, T.GELU))
def test_references_against_autograd(act):
    """Forward against F.conv2d of the concatenated, activated input; the data gradient against autograd through it and against
    conv_transpose2d, in f64."""
    c = _small("fwd", "f32", act, res1=True, res2=True)
    I = R.make_inputs(c)
    fn = {T.NONE: lambda t: t, T.RELU: torch.relu, T.GELU: F.gelu}[act]
    x = torch.cat(I.segs, -1).permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.conv2d(fn(x), I.wq, I.bias.double(), padding=1)
    want = y + (I.res1 + I.res2).permute(0, 3, 1, 2)
    got = R.reference(c, I)
    assert torch.allclose(got.ref.permute(0, 3, 1, 2), want, rtol=0, atol=1e-13)
    assert (got.A >= got.ref.abs() - 1e-13).all()
    for k in (0, 1):
        d = _small("dgrad", "f32", act, bias=False, res1=True, k=k)
        J = R.make_inputs(d)
        xs = [torch.randn(2, ck, 5, 6, dtype=torch.float64) for ck in d.segs]
        xs[k] = J.aux.permute(0, 3, 1, 2).clone() if act else xs[k]
        xs = [t.requires_grad_(True) for t in xs]
        out = F.conv2d(fn(torch.cat(xs, 1)), J.wq, None, padding=1)
        g = J.segs[0].permute(0, 3, 1, 2)
        (gx,) = torch.autograd.grad(out, xs[k], g)
        got = R.reference(d, J)
        assert torch.allclose(got.ref.permute(0, 3, 1, 2), gx + J.res1.permute(0, 3, 1, 2), rtol=0, atol=1e-13)
        ct = F.conv_transpose2d(g, J.wq[:, d.seg_off:d.seg_off + d.out_c], padding=1)
        assert torch.allclose(F.conv2d(g, R.effective_weight(d, J), padding=1), ct, rtol=0, atol=1e-13)


def test_relu_derivative_at_zero_and_planted_values():
    c = _small("dgrad", "h16", T.RELU, bias=False)
    I = R.make_inputs(c)
    aux = I.aux.view(-1)
    zeros = aux == 0
    assert int(zeros.sum()) >= 2 and bool(torch.signbit(aux[zeros]).any()) and not bool(torch.signbit(aux[zeros]).all())  # +0.0 and -0.0
    assert bool((aux == R.smallest_positive(I.tdt)).any())
    assert bool((R.reference(c, I).ref.view(-1)[zeros] == 0).all())  # relu'(+-0) = 0
    g = _small("fwd", "h16", T.GELU)
    assert float(R.make_inputs(g).segs[0].abs().max()) == 8.0


@pytest.mark.parametrize("C", (1, 3))
def test_reference_against_the_recorded_likelihood_head(C):
    """tests/golden/ops.pt holds 1x1 convs run by the reference implementation: x_loc of the DGauss heads, 8 -> C channels, whose output
    is the recorded `loc` -- every channel of the grey head, channel 0 of the RGB head (its channels 1 and 2 are mixed with the true
    pixels by channel_coeffs afterwards).  The recorded values are torch's f32 conv: held to the a-priori 2 L + 1 roundings."""
    d = load_golden("ops.pt")[f"dgauss_c{C}"]
    c = T.Case("fwd", "f32", 4, 9, 9, (8,), C, 1)
    I = R.Inputs()
    I.tdt = torch.float32
    I.segs = [d["h"].permute(0, 2, 3, 1).double()]
    I.w = d["state_dict"]["x_loc.weight"]
    I.wq, I.bias = I.w.double(), d["state_dict"]["x_loc.bias"]
    I.aux = I.res1 = I.res2 = I.res1_rem = None
    got = R.reference(c, I)
    keep = slice(0, 1)  # (channel 0 is the plain conv in both heads)
    rec = d["loc"].permute(0, 2, 3, 1)
    assert_bounded(rec[..., keep], got.ref[..., keep], got.A[..., keep], 2 * c.L() + 1, torch.float32)
    assert float((rec[..., keep].double() - got.ref[..., keep]).abs().max()) < 1e-5 * float(got.A.max())


GELU16 = [c for c in CASES if c.dir == "fwd" and c.act == T.GELU and c.dt == "h16"]


@pytest.mark.parametrize("bf16", (False, True))
@pytest.mark.parametrize("case", GELU16, ids=lambda c: c.id())
def test_flagged_share_of_16bit_gelu_operands(case, bf16):
    I = R.make_inputs(case, bf16)
    a, _, shift, share = R.activated(case, I)
    assert 0 < share <= R.FLAG_SHARE_MAX, share
    assert bool(((shift > 0) == (shift >= torch.maximum(*[(n - a).abs() for n in R._neighbours(a.to(I.tdt))]))).all())


def test_recorded_k_acc_holds():
    """Re-measured on a subset: the three cases of every family with the longest K and its first three."""
    by = {}
    for c in CASES:
        by.setdefault(T.family(c), []).append(c)
    assert set(by) == set(R.K_ACC)
    for fam, cs in by.items():
        sub = sorted(cs, key=lambda c: -c.L())[:3] + cs[:3]
        worst = max(R.chain_error(c, R.make_inputs(c), budget=1 << 20) for c in sub)
        assert 0.5 < worst and R.K_MARGIN * worst <= R.K_ACC[fam], (fam, worst)
    c = _small("fwd", "f32", T.NONE)
    c1 = T.Case("fwd", "f32", 1, 1, 1, (1,), 1, 1)
    assert R.reference(c1, R.make_inputs(c1)).k_acc == 2.0  # never more than the a-priori 2 L
    assert R.reference(c, R.make_inputs(c)).k_acc == R.K_ACC[T.family(c)]


# --------------------------------------------------------------------------------------------------------------- the mutants
_APPLIED = {}  # case id -> the mutants that applied (filled by _check_mutants)


def _check_mutants(case):
    I = R.make_inputs(case)
    ref = R.reference(case, I)
    assert_bounded(ref.ref.to(I.tdt), ref.ref, ref.A_tol, ref.k, I.tdt)
    assert bool(torch.isfinite(ref.ref).all()) and bool((ref.A_tol >= 0).all())
    applied = []
    for m in R.MUTANTS:
        mr = R.reference(case, I, m)
        if mr is None or torch.equal(mr.ref, ref.ref):
            continue
        applied.append(m)
        with pytest.raises(AssertionError, match="outside the k="):
            assert_bounded(mr.ref.to(I.tdt), ref.ref, ref.A_tol, ref.k, I.tdt)
    _APPLIED[case.id()] = applied
    return applied


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id())
def test_bound_sees_every_mutant(case):
    """Each applicable mutant of the f64 reference, rounded to the output format, fails the bound the kernels are held to; the
    reference itself, rounded, passes it.  A mutant applies where it changes the reference (dropping a corner tap of a one-row image
    does not)."""
    _check_mutants(case)


def test_every_mutant_applies_on_every_arm():
    for m in R.MUTANTS:
        dirs = ("dgrad",) if m in ("no_flip", "shift_dact") else (("fwd",) if m in ("drop_res2", "drop_bias_last_group") else ("fwd", "dgrad"))
        for d in dirs:
            for a in ("gen", "tile", "px", "ws", "smlp"):
                assert any(m in (_APPLIED.get(c.id()) or _check_mutants(c)) for c in _of(a, dir=d)), (m, d, a)
