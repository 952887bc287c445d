"""Without a GPU: the case tables of tests/test_gpu_latent_like.py reach every arm of every latent / likelihood / ELBO entry point in
both dtypes and every boundary the kernels have; the directed values sit on the branches they are meant for; the f64 references
reproduce the recorded reference output they overlap (tests/golden/ops.pt, dmol_lowbit.pt); no case leaves more than 0.5 % of its
elements uncompared; and the recorded K of every family covers torch's own f32 run of the same formulas."""
import math
import os
import re
from collections import defaultdict

import pytest
import torch
import torch.nn.functional as F

import latent_like_cases as T
import latent_like_ref as R
from conftest import ROOT, load_golden


def _tdt(case):
    """The storage dtype of a case in THIS build (asking the library needs no GPU)."""
    if case.dt == "f32":
        return torch.float32
    from causal_gen_amd import _lib

    return torch.bfloat16 if _lib.load().h16_is_bf16 else torch.float16


def _of(op, **kw):
    return [c for c in T.CASES if c.op == op and all(getattr(c, k) == v for k, v in kw.items())]


def test_case_ids_are_unique():
    ids = [c.id() for c in T.CASES]
    assert len(ids) == len(set(ids))
    assert all(T.FAMILY[c.op] for c in T.CASES)


@pytest.mark.parametrize("op", T.LATENT_OPS + T.LIKE_OPS + T.ELBO_OPS)
def test_every_arm_is_reached(op):
    assert {T.arm(c) for c in _of(op)} == T.arms_of(op), op


def test_latent_chunk_boundaries_and_layouts():
    for op in ("reparam_kl_fwd", "reparam_kl_bwd"):
        for dt in T.DTYPES:
            cs = _of(op, dt=dt)
            for n in (1, 3):
                assert {T.per(c) for c in cs if c.n == n} >= {1, 2047, 2048, 2049, 4920}, (op, dt, n)
            assert any(T.lat_chunks(c) == 3 and T.per(c) % T.LAT_CHUNK for c in cs)  # two whole chunks and a part
        h16 = _of(op, dt="h16")
        scalar = [c for c in h16 if T.arm(c) == "h16-scalar"]
        vec8 = [c for c in h16 if T.arm(c) == "h16-vec8"]
        assert {c.c for c in scalar} >= {3, 12} and any(c.c == 16 and c.off == 4 for c in scalar)  # by c % 8, and by 8-byte alignment
        assert {c.c for c in vec8} >= {8, 16, 24} and {c.off for c in vec8} >= {0, 8}
        assert any(c.off and c.cext for c in vec8)  # 16-byte stores into a slice: the neighbouring channels must survive
    fwd = _of("reparam_kl_fwd")
    for a in T.arms_of("reparam_kl_fwd"):
        assert {(c.get("eps_out"), c.get("logt") != 0.0) for c in fwd if T.arm(c) == a} == {(0, False), (0, True), (1, False), (1, True)}, a


def test_reparam_kl_bwd_arguments():
    bwd = _of("reparam_kl_bwd")
    for a in T.arms_of("reparam_kl_bwd"):
        cs = [c for c in bwd if T.arm(c) == a and not T.wraps(c)]
        assert {(c.get("acc_q"), c.get("acc_p")) for c in cs} == {(0, 0), (0, 1), (1, 0), (1, 1)}, a
        for key in ("gz", "cs", "coef_stride"):
            for v in (0, 1):  # each value of each optional argument meets acc_q != acc_p both ways round
                assert {(c.get("acc_q"), c.get("acc_p")) for c in cs if c.get(key) == v} >= {(0, 1), (1, 0)}, (a, key, v)
        assert any(c.get("coef_stride") == 1 and c.n > 1 for c in cs)
        assert any(c.get("cs") and c.c >= 3 for c in cs)  # chan_scale entries 0, 0.5 and 1 all occur
        wrapped = [c for c in bwd if T.arm(c) == a and T.wraps(c)]
        assert len(wrapped) == 1 and T.work_items(wrapped[0]) > 4096 * 256, a
    assert any(c.n == 3 and (c.h, c.w, c.c) == (60, 61, 96) and c.dt == "f32" for c in bwd)
    assert any(c.n == 2 and (c.h, c.w, c.c) == (128, 129, 256) and T.arm(c) == "h16-vec8" for c in bwd)
    rid = _of("reparam_kl_bwd_rider")
    assert {(c.get("ride_c"), c.get("ride_acc")) for c in rid} == {(8, 0), (8, 1), (32, 0), (32, 1)}
    for c in rid:  # the rider's own views keep the 16-byte path
        assert T.lat_vec8_ok(c.n, c.get("ride_c"), [T.view_layout(c, (c.n, c.h, c.w, c.get("ride_c")))])


def test_other_latent_cases():
    for dt in T.DTYPES:
        med = _of("mediator_mix", dt=dt)
        for hw in (True, False):
            cs = [c for c in med if (c.h * c.w == 1) == hw]
            assert {(c.get("linear_var"), c.get("alpha"), c.get("t")) for c in cs} == {(lv, a, t) for lv in (0, 1) for a in (0.0, 0.3, 1.0) for t in (0.0, 0.7)}
        ks = _of("kl_channel_sums", dt=dt)
        assert {c.c for c in ks} == {1, 2, 16, 64, 256}
        for c_ in (1, 2, 16, 64, 256):
            L = 256 // c_
            assert {c.h * c.w for c in ks if c.c == c_} == {v for v in (1, L - 1, L + 1, 3 * L + 1) if v > 0}
        assert all(c.get("out_extra") > 0 for c in ks)
        assert _of("sample_gaussian", dt=dt)
    assert {c.c for c in _of("gaussian_kl_map")} == {0, 1, 255, 257, 4096 * 256 + 3}


def test_likelihood_boundaries():
    pix = {1, 1023, 1024, 1025, 2115}
    for dt in T.DTYPES:
        for op in ("dgauss_nll_fwd", "dgauss_nll_bwd"):
            cs = _of(op, dt=dt)
            for n in (1, 3):
                for (C, pc) in ((1, 2), (3, 9), (3, 6)):
                    assert {c.h * c.w for c in cs if c.n == n and c.c == C and c.get("pc") == pc and not c.off and not T.wraps(c) and not c.get("only")} == pix, (op, dt, n, C, pc)
            assert any(c.off and c.cext and c.c == 1 for c in cs) and any(c.off and c.cext and c.get("pc") == 9 for c in cs)
        assert {c.get("coef_stride") for c in _of("dgauss_nll_bwd", dt=dt) if c.n == 3} == {0, 1}
        assert {(c.c, c.get("x")) for c in _of("dgauss_params", dt=dt)} == {(1, 0), (1, 1), (3, 0), (3, 1)}
        assert all(c.get("logt") != 0.0 and c.off for c in _of("dgauss_params", dt=dt))
        assert {c.get("pc") for c in _of("dgauss_sample", dt=dt)} == {2, 6, 9}
        assert {(c.c, c.get("pc")) for c in _of("cf_dgauss_bwd", dt=dt)} >= {(1, 2), (3, 9), (3, 12)}
        for op in ("gauss_nll_fwd", "gauss_nll_bwd"):
            cs = _of(op, dt=dt)
            cs = [c for c in cs if not c.get("only")]
            assert {c.h * c.w for c in cs} == pix and {c.c for c in cs} == {1, 3} and {c.n for c in cs} == {1, 3}
            for C in (1, 3):
                assert {c.h * c.w for c in cs if c.c == C} >= {1023, 1025}
        for op in ("dmol_nll_fwd", "dmol_nll_bwd"):
            for low in (0, 1):
                assert {c.h * c.w for c in _of(op, dt=dt) if c.get("low_bit") == low and not c.get("only")} == {1, 1023, 1025}
    w = [c for c in T.LIKE_CASES if T.wraps(c)]
    assert [(c.op, c.c, c.n, c.h, c.w) for c in w] == [("dgauss_nll_bwd", 1, 5, 459, 457)]


def test_elbo_boundaries():
    fin = _of("elbo_finalize")
    assert {c.n for c in fin} == {1, 15, 16, 17, 33, 100}  # the 16-wave stride
    assert {c.get("nll_count") for c in fin} == {1, 63, 64, 65, 130} and {c.get("kl_count") for c in fin} == {0, 1, 64, 200}  # the 64 lanes
    assert {c.get("beta_dev") for c in fin} == {0, 1}
    assert {c.n > 16 for c in fin if c.get("kl_count") == 0} == {True, False}  # the null kl_part on both sides of the wave stride
    fb = _of("elbo_finalize_fb")
    assert {c.n for c in fb} == {1, 8, 300} and {c.get("ncol") for c in fb} == {1, 255, 256, 257, 700}  # the 256-thread column stride
    assert {c.get("cols") for c in fb} == {"above", "below", "mixed", "tie"}
    assert all(c.n == 8 for c in fb if c.get("cols") == "tie")
    for c in (c for c in fb if c.get("cols") == "tie"):
        o = R.reference(c, R.make_inputs(c, torch.float32))["chan_mask"]
        assert (o.ref == 0.5).all()  # every entry 0.25, n = 8: the column mean is free_bits exactly, in f32 and in f64


def test_mirror_matches_the_host_code():
    """lat_vec8_ok, the chunk sizes and the grid cap are copied from the kernels' sources; a change there must be carried over."""
    lat = open(os.path.join(ROOT, "causal-gen_amd", "csrc", "latent.hip")).read()
    bodies = open(os.path.join(ROOT, "causal-gen_amd", "csrc", "latent_bodies.inc")).read()
    like = open(os.path.join(ROOT, "causal-gen_amd", "csrc", "likelihood.hip")).read()
    common = open(os.path.join(ROOT, "causal-gen_amd", "csrc", "common.h")).read()
    v8 = re.search(r"static inline bool lat_vec8_ok\(.*?\n}\n", lat, re.S).group(0)
    assert "if (c % 8) return false;" in v8 and "if (!cgen::vec16_ok(v, 2)) return false;" in v8
    assert "if ((int64_t)n * v.sn >= ((int64_t)1 << 31)) return false;" in v8
    assert "return (((uintptr_t)v.p) % 16 == 0) && ((v.sn * esz) % 16 == 0) && ((v.sh * esz) % 16 == 0) && ((v.sw * esz) % 16 == 0);" in common
    assert "#define LAT_CHUNK 2048" in bodies and "#define LIKE_PIX 1024" in like
    assert lat.count("(b > 4096 ? 4096 : b)") == 1 and like.count("(b > 4096 ? 4096 : b)") == 1  # lat_grid, like_grid
    assert "for (int b = wave; b < n; b += 16)" in like and "for (int j = threadIdx.x; j < ncol; j += 256)" in like
    assert "#define DG_MIN_LS (-9.0f)" in like and "#define DM_MIN_LS (-7.0f)" in like


def test_mirror_decisions():
    assert T.lat_vec8_ok(3, 8, [(0, 8 * 48, 8 * 6, 8)]) and not T.lat_vec8_ok(3, 12, [(0, 16 * 48, 16 * 6, 16)])
    assert not T.lat_vec8_ok(3, 16, [(8, 24 * 48, 24 * 6, 24)])  # 16 channels at offset 4: 8-byte aligned
    assert not T.lat_vec8_ok(3, 8, [(0, 12 * 48, 12 * 6, 12)])  # pixel stride of 24 bytes
    assert not T.lat_vec8_ok(2, 8, [(0, 1 << 30, 8, 8)])  # n * sn past 31 bits


# ------------------------------------------------------------------------------------------------------- directed values
def _first(op, dt, **kw):
    return next(c for c in _of(op, dt=dt) if c.n * c.h * c.w >= 24 and all(c.get(k) == v for k, v in kw.items()))


@pytest.mark.parametrize("dt", T.DTYPES)
def test_dgauss_directed_values(dt):
    for pc, C in ((2, 1), (9, 3)):
        c = next(c for c in _of("dgauss_nll_bwd", dt=dt) if c.n * c.h * c.w >= 24 and c.c == C and c.get("pc") == pc and c.get("coef_stride") == 0)
        tdt = _tdt(c)
        inp = R.make_inputs(c, tdt)
        x, p = inp["x"].double().reshape(-1, C), inp["params"].double().reshape(-1, pc)
        assert x[0, 0] == -1 and x[1, 1 % C] == 1 and (x[2, 2 % C] - (1 - 2 / 255)).abs() < 4e-3 and (x[3, 0] + (1 - 2 / 255)).abs() < 4e-3
        lo, hi = R.storage_ulp(tdt, -9.0, True), R.storage_ulp(tdt, -9.0, False)
        assert lo < -9.0 < hi and p[4:8, C].tolist() == [-9.0, lo, hi, -20.0]
        g = R.reference(c, inp)["g"]
        gr, A = g.ref.reshape(-1, pc), g.A.reshape(-1, pc)
        assert not g.excl.reshape(-1, pc)[:9].any() and inp["directed"].flatten()[:9].all()
        # at the clamp and above it the log-scale gradient passes (and is far from zero: `>` for `>=` would show); below it is exactly 0
        assert gr[4, C].abs() > 1e-4 and gr[6, C].abs() > 1e-4 and gr[5, C] == 0 and gr[7, C] == 0
        assert torch.allclose(gr[4, C], gr[6, C], rtol=0.1) and A[5, C] == 0
        # the whole bound at the tie (most of it the saturated upper CDF's 1 - t^2 on absolute values) stays under half the gradient:
        # a kernel that returns 0 there is outside it
        ulp1 = float(R.storage_ulp(tdt, 1.0, False) - 1.0) if tdt != torch.float32 else 0.0
        assert R.K["dgauss"] * R.U32 * A[4, C] + ulp1 * gr[4, C].abs() < 0.5 * gr[4, C].abs()
        # the far-tail pixel: under the 1e-12 floor, -log 1e-12 and both gradients exactly 0
        assert gr[8, 0] == 0 and gr[8, C] == 0 and A[8, 0] == 0
        f = next(k for k in _of("dgauss_nll_fwd", dt=dt) if (k.n, k.h, k.w, k.c, k.p[0]) == (c.n, c.h, c.w, c.c, c.p[0]) and k.off == c.off)
        term = R.reference(f, R.make_inputs(f, tdt))["nll_part"].terms[0].reshape(-1, C)
        assert abs(float(term[8, 0]) + math.log(1e-12)) < 1e-12


@pytest.mark.parametrize("dt", T.DTYPES)
def test_gauss_and_cf_directed_values(dt):
    c = next(c for c in _of("gauss_nll_bwd", dt=dt) if c.n * c.h * c.w >= 24 and c.c == 3)
    tdt = _tdt(c)
    inp = R.make_inputs(c, tdt)
    assert inp["x"].reshape(-1, 3)[0, 0] == -1 and inp["u"].reshape(-1, 3)[0, 0] == 0
    _, v, tgt, _, _ = R.gauss_terms(inp["params"].double(), inp["x"].double(), inp["u"].double(), 3)
    assert v.reshape(-1, 3)[0, 0] == R.F32_TINY and abs(float(tgt.reshape(-1, 3)[0, 0]) - math.log(R.F32_TINY)) < 1e-9  # the tiny clamp
    p = inp["params"].double().reshape(-1, 6)
    assert p[1:5, 3].tolist() == [-9.0, R.storage_ulp(tdt, -9.0, True), R.storage_ulp(tdt, -9.0, False), -20.0]
    g = R.reference(c, inp)["g"].ref.reshape(-1, 6)
    assert g[1, 3] != 0 and g[3, 3] != 0 and g[2, 3] == 0 and g[4, 3] == 0
    for pc in (9, 12):
        c = next(c for c in _of("cf_dgauss_bwd", dt=dt) if c.get("pc") == pc)
        inp = R.make_inputs(c, tdt)
        ref = R.reference(c, inp)
        rpre, cpre, y = R._cf_forward(inp["params"].double(), inp["cf"].double(), inp["x"].double(), 3, True)
        y, rpre, cpre = y.reshape(-1, 3), rpre.reshape(-1, 3), cpre.reshape(-1, 3)
        assert y[9, 0] < -1 and y[10, 0] > 1  # y outside [-1, 1]: no gradient through the outer clamp
        k = 11
        for pre in (rpre, cpre):
            for ch in range(3):
                assert pre[k, ch] < -1 and pre[k + 1, ch] > 1  # each pre-clamp mean of each head outside [-1, 1]
                k += 2
        assert k == 23 and inp["directed"].flatten()[:23].all()
        assert all(float(o.excl.double().mean()) <= 0.005 for o in ref.values())
        g = ref["g_cf"].ref.reshape(-1, pc)
        # y of channel 0 outside: nothing reaches its scale; a pre-clamp mean 0 outside (pixel 17: cf's, pixel 11: rec's): nothing passes it
        assert g[9, 3] == 0 and g[17, 0] == 0 and ref["g"].ref.reshape(-1, pc)[11, 0] == 0
        if pc == 12:
            assert not ref["g"].ref[..., 9:].any() and not ref["g_cf"].ref[..., 9:].any() and not ref["g"].A[..., 9:].any()


@pytest.mark.parametrize("dt", T.DTYPES)
@pytest.mark.parametrize("low", [0, 1])
def test_dmol_directed_values_and_the_tie(dt, low):
    c = next(c for c in _of("dmol_nll_bwd", dt=dt) if c.n * c.h * c.w >= 24 and c.get("low_bit") == low)
    tdt = _tdt(c)
    inp = R.make_inputs(c, tdt)
    l, x = inp["params"].double().reshape(-1, 100), inp["x"].double().reshape(-1, 3)
    assert x[0, 0] == -1 and x[1, 1] == 1
    lo, hi = R.storage_ulp(tdt, -7.0, True), R.storage_ulp(tdt, -7.0, False)
    assert l[4:8, 20].tolist() == [-7.0, lo, hi, -20.0]
    g = R.reference(c, inp)["g"]
    gr = g.ref.reshape(-1, 100)
    assert not g.excl.reshape(-1, 100)[:10].any()
    # component 0 carries pixels 4..7 and its R log-scale gradient is far from 0 above the clamp; on the tie it is one half of the
    # pass-through gradient (the pixels differ only in that log-scale, by one storage ulp), below the clamp exactly 0
    assert gr[6, 20].abs() > 1e-4 and gr[5, 20] == 0 and gr[7, 20] == 0
    assert torch.allclose(gr[4, 20], 0.5 * gr[6, 20], rtol=0.15)  # (a bf16 ulp at 7 moves the scale by 3 %; a wrong rule is off by 100 %)
    # pixels 8, 9: every R component in the delta <= 1e-5 fallback, and the pixel's gradients alive
    hb = R.HB5 if low else R.HB8
    _, means, lsr, _ = R.dmol_ref._unpack(inp["params"].double())
    d = x[8:10, 0, None] - means.reshape(-1, 3, 10)[8:10, 0]
    delta = torch.sigmoid((d + hb) * (-lsr.reshape(-1, 3, 10)[8:10, 0]).exp()) - torch.sigmoid((d - hb) * (-lsr.reshape(-1, 3, 10)[8:10, 0]).exp())
    assert (delta <= 1e-5).all() and (gr[8:10, 10:20].abs().sum(1) > 1e-4).all()


def test_the_oracle_halves_the_gradient_on_a_tie():
    """torch.max(t, -7 * ones) as in the reference's const_max: all above, none below, one half at equality."""
    torch.manual_seed(0)
    l0 = torch.randn(1, 1, 1, 100, dtype=torch.float64) * 0.5
    x = torch.tensor([[[[26.0, -51.0, 77.0]]]], dtype=torch.float64) / 127.5
    l0[..., 0], l0[..., 10] = 5.0, x[..., 0]
    g = {}
    for name, v in (("tie", -7.0), ("above", -7.0 + 1e-9), ("below", -7.0 - 1e-9)):
        l = l0.clone()
        l[..., 20] = v
        l.requires_grad_(True)
        R.dmol_ref.dmol_nll(x, l).sum().backward()
        g[name] = l.grad[0, 0, 0, 20].item()
    assert g["below"] == 0 and g["above"] != 0 and abs(g["tie"] / g["above"] - 0.5) < 1e-6


@pytest.mark.parametrize("dt", T.DTYPES)
def test_forward_chunks_of_directed_pixels_see_a_wrong_branch(dt):
    """The cases that hold the directed pixels alone: the whole bound of their one forward chunk is under a fifth of what a removed
    log-scale clamp (-9 / -7 -> -30) changes in it, and, for the discretised Gaussian, of what a floor of 1e-10 for 1e-12 would
    (log 100 at the far-tail pixel, whose own amplification is |log 1e-12| alone)."""
    from oracle import dmol_ref, hvae_ref, simple_ref

    cases = [c for c in T.LIKE_CASES if c.get("only") and c.op.endswith("nll_fwd") and c.dt == dt]
    assert {c.op for c in cases} == {"dgauss_nll_fwd", "gauss_nll_fwd", "dmol_nll_fwd"} and len(cases) == 4
    for c in cases:
        inp = R.make_inputs(c, _tdt(c))
        assert inp["directed"].all()
        o = R.reference(c, inp)["nll_part"]
        assert o.ref.numel() == 1 and not o.excl.any() if o.excl is not None else o.ref.numel() == 1
        tol = float(R.K[T.FAMILY[c.op]] * R.U32 * o.A + R.U32 * o.S)
        saved = hvae_ref.MIN_LOGSCALE, simple_ref.EPS, dmol_ref.MIN_LOG_SCALE
        try:
            hvae_ref.MIN_LOGSCALE = simple_ref.EPS = dmol_ref.MIN_LOG_SCALE = -30.0
            change = float((R.reference(c, inp)["nll_part"].ref - o.ref).abs())
        finally:
            hvae_ref.MIN_LOGSCALE, simple_ref.EPS, dmol_ref.MIN_LOG_SCALE = saved
        assert change > 0.3 and tol < 0.2 * change, (c.id(), tol, change)
        if c.op == "dgauss_nll_fwd":
            term, A = o.terms
            assert abs(float(term.flatten()[8]) + math.log(1e-12)) < 1e-12 and abs(float(A.flatten()[8]) + math.log(1e-12)) < 1e-9
            assert tol < 0.2 * math.log(100.0)
        if c.op == "gauss_nll_fwd":  # x = -1, u = 0: the target is the constant log(tiny), its bound a few hundred units, not 1e40
            assert float(o.terms[1].flatten()[0]) < 1e4


# ------------------------------------------------------------------------------------------------------- golden anchors
def _within(got64, golden32, A, fam, excl=None):
    """The recorded f32 reference output lies inside the family's bound around the f64 reference (but for the elements next to a
    branch threshold, where the recorded f32 run may have taken the other branch)."""
    err = (got64 - golden32.double()).abs()
    if excl is not None:
        assert float(excl.double().mean()) <= 0.05  # (the fixtures' draws are not the tables': 4 of dmol_lowbit.pt's 147 pixels)
        err = err * ~excl
    bad = ~(err <= R.K[fam] * R.U32 * A + 1e-30)  # (+ 1e-30: far-tail components of the recorded f32 run pass through subnormals)
    assert not bad.any(), (float((err / (R.U32 * A))[bad].max()), got64[bad][:4], golden32[bad][:4])


def test_references_reproduce_the_golden_fixtures():
    ops = load_golden("ops.pt")
    fx = ops["gaussian_kl"]
    flat = {k: fx[k2].reshape(-1) for k, k2 in (("q_loc", "q_loc"), ("q_ls", "q_logscale"), ("p_loc", "p_loc"), ("p_ls", "p_logscale"))}
    o = R.reference(T.Case("gaussian_kl_map", "f32", 1, 1, 1, flat["q_loc"].numel()), flat)["out"]
    _within(o.ref, fx["kl"].reshape(-1), o.A, "latent")
    for C in (1, 3):
        d = ops[f"dgauss_c{C}"]
        sd, x = d["state_dict"], d["x"]
        N, _, H, W = x.shape
        names = ["x_loc", "x_logscale"] + (["channel_coeffs"] if C == 3 else [])
        raw = torch.cat([F.conv2d(d["h"], sd[f"{n}.weight"], sd[f"{n}.bias"]) for n in names], dim=1).permute(0, 2, 3, 1).contiguous()
        inp = {"params": raw, "x": x.permute(0, 2, 3, 1).contiguous(), "directed": torch.zeros(N, H, W, dtype=torch.bool)}
        case = T.Case("dgauss_nll_fwd", "f32", N, H, W, C, p=T.P(pc=raw.shape[-1]))
        o = R.reference(case, inp)["nll_part"]
        _within(o.ref.sum(1) / (C * H * W), d["nll"], (o.A.sum(1) + o.S.sum(1)) / (C * H * W), "dgauss")
        s = R.reference(T.Case("dgauss_sample", "f32", N, H, W, C, p=T.P(pc=raw.shape[-1])), inp)
        _within(s["x"].ref, d["sample_x"], s["x"].A + 1e-30, "dgauss")
        _within(s["scale"].ref, d["sample_scale"], s["scale"].A, "dgauss")
        pr = R.reference(T.Case("dgauss_params", "f32", N, H, W, C, p=T.P(pc=raw.shape[-1], x=1, logt=0.0)), inp)
        _within(pr["loc"].ref, d["loc"], pr["loc"].A + 1e-30, "dgauss")
        _within(pr["ls"].ref, d["logscale"], pr["ls"].A, "dgauss")
    for d, low, key in ((ops["dmol"], 0, "loss"), (load_golden("dmol_lowbit.pt"), 1, "loss"), (load_golden("dmol_lowbit.pt"), 0, "loss_8bit")):
        N, H, W, _ = d["l"].shape
        D = 3 * H * W
        inp = {"params": d["l"], "x": d["x"], "directed": torch.zeros(N, H, W, dtype=torch.bool), "coef": torch.tensor([1.0 / D])}
        o = R.reference(T.Case("dmol_nll_fwd", "f32", N, H, W, 3, p=T.P(low_bit=low)), inp)["nll_part"]
        _within(o.ref.sum(1) / D, d[key], (o.A.sum(1) + o.S.sum(1)) / D, "dmol")
        if key == "loss":
            g = R.reference(T.Case("dmol_nll_bwd", "f32", N, H, W, 3, p=T.P(low_bit=low, coef_stride=0)), inp)["g"]
            _within(g.ref, d["grad_l"], g.A, "dmol", g.excl)


def test_gauss_terms_is_the_oracle_formula():
    """gauss_terms restates simple_ref.gauss_nll with the f32 clamp constants spelt out (the oracle takes them from the dtype it
    runs in): in f32 the two agree to rounding."""
    g = torch.Generator().manual_seed(3)
    N, C, H, W = 3, 3, 6, 5
    raw = torch.randn(N, 2 * C, H, W, generator=g) * 0.5
    x = (torch.randint(0, 256, (N, C, H, W), generator=g).float() - 127.5) / 127.5
    u = torch.rand(N, C, H, W, generator=g)
    x[0, 0, 0, 0], u[0, 0, 0, 0] = -1.0, 0.0
    want = simple_gauss = R.simple_ref.gauss_nll(R._identity_heads(C, 2 * C, torch.float32, "cpu"), raw, x, u)
    nhwc = lambda t: t.permute(0, 2, 3, 1)  # noqa: E731
    got = R.gauss_terms(nhwc(raw), nhwc(x), nhwc(u), C)[0].sum(dim=(1, 2, 3)) / (C * H * W)
    torch.testing.assert_close(got, want, rtol=2e-6, atol=0)
    assert simple_gauss.shape == (N,)


# ------------------------------------------------------------------------------------- the exclusion cap and the recorded K
@pytest.mark.parametrize("fam", ["latent", "dgauss", "gauss", "dmol", "elbo"])
def test_exclusion_cap_and_recorded_k(fam):
    worst = defaultdict(float)
    for c in T.CASES:
        if T.FAMILY[c.op] != fam:
            continue
        assert R.excluded_fraction(c, _tdt(c)) <= 0.005, c.id()
        if fam != "elbo":
            worst[fam] = max(worst[fam], R.measure_k(c, _tdt(c)))
    if fam != "elbo":
        # the record covers the measurement and is not inflated (the measurement moves a little with the build's 16-bit format)
        assert 0.25 * R.K_MEASURED[fam] <= worst[fam] <= R.K_MEASURED[fam], (fam, worst[fam])
