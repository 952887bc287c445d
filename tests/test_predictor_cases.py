"""The case table of tests/test_gpu_predictor_sites.py without a GPU: the mirror of the tiled placement's host side against the
library (workspace sizes, the fused placement's LDS test, the plan entry over every width and resolution), the coverage claims over
the full (width, R) sweep, the chained local references against f64 autograd of the whole network, pred_nll's branch points, the
recorded accumulation constants against a fresh measurement, and every mutant rejected where it applies."""
import ctypes
import math

import pytest
import torch

import predictor_cases as pc
import predictor_site_ref as ref
from predictor_cases import BWD, CASES, FWD, MIXED, R_CASE_MAX, STEM_BWD, UNREACHABLE, WIDTHS

# edges the sweep first shows above R_CASE_MAX: named, not covered (a 3x3 layer without the pool in front reaches several
# 16-pixel tiles only from R = 259 on)
EDGES_NOT_COVERED = {(("ptile_conv_fwd", 3, 2, 2, 8, False), "multi"): 259, (("ptile_conv_fwd", 3, 2, 2, 8, False), "ragged"): 259}


def _recs(c, r, widths):
    from causal_gen_amd import _lib

    recs = (_lib.PredHead * len(widths))()
    for h, w in zip(recs, widths):
        h.c, h.res, h.width, h.nout, h.kind, h.obs_stride = c, r, w, 2, _lib.PRED_NORMAL, 1
    return recs


def _lib_plan(lib, c, r, w, n, nheads):
    from causal_gen_amd import _lib

    rec = (_lib.i32 * (8 * 16))(*([-1] * 128))
    count = _lib.i32(0)
    lib.predictor_tiled_plan(_recs(c, r, [w] * nheads), nheads, n, rec, 16, ctypes.byref(count))
    return [tuple(rec[8 * i:8 * i + 8]) for i in range(count.value)], list(rec[8 * count.value:])


def test_mirror_matches_the_library_over_every_width_and_resolution():
    from causal_gen_amd import _lib

    lib = _lib.load()
    for w in WIDTHS:
        for r in range(pc.R_MIN, pc.R_MAX + 1):
            got, rest = _lib_plan(lib, 1, r, w, 2, 3)
            assert got == [tuple(l) for l in pc.plan(1, r, w, 2, 3)], (r, w)
            assert set(rest) == {-1}  # nothing written past the records
    for c in CASES:
        nh = len(c.heads)
        need = _lib.i64(0)
        lib.predictor_tiled_workspace(_recs(c.C, c.R, [c.width] * nh), nh, c.n, ctypes.byref(need))
        assert need.value == c.n * nh * pc.pred_geo(c.C, c.R, c.width).total, c.tag
    for c in CASES + MIXED:
        widths = [pc.head_width(c, h) for h in c.heads]
        per = _lib.i64(0)
        lib.predictor_workspace(_recs(c.C, c.R, widths), len(widths), ctypes.byref(per))
        assert per.value == max(pc.pred_geo(c.C, c.R, w).total for w in widths), c.tag
        assert lib._raw_cgen_predictor_supported(_recs(c.C, c.R, widths), len(widths)) == int(pc.fused_ok(c.C, c.R, widths)), c.tag


def test_plan_entry_arguments():
    from causal_gen_amd import _lib

    lib = _lib.load()
    count = _lib.i32(0)
    lib.predictor_tiled_plan(_recs(1, 40, [8]), 1, 1, None, 0, ctypes.byref(count))  # records are optional
    assert count.value == 13
    rec = (_lib.i32 * 16)(*([-1] * 16))
    lib.predictor_tiled_plan(_recs(1, 40, [8]), 1, 1, rec, 1, ctypes.byref(count))  # a short buffer gets the first records only
    assert count.value == 13 and tuple(rec[:8]) == tuple(pc.plan(1, 40, 8, 1, 1)[0]) and set(rec[8:]) == {-1}
    for bad, words in (((_recs(1, 40, [8, 16]), 2, 1), "does not take these heads"), ((_recs(1, 4, [8]), 1, 1), "does not take these heads"),
                       ((_recs(1, 40, [8]), 1, 0), "bad batch")):
        with pytest.raises(_lib.CgenError, match=words):
            lib.predictor_tiled_plan(*bad, rec, 2, ctypes.byref(count))
    with pytest.raises(_lib.CgenError, match="null count"):
        lib.predictor_tiled_plan(_recs(1, 40, [8]), 1, 1, rec, 2, None)


def _coverage():
    cov = {}
    for c in CASES:
        g = pc.pred_geo(c.C, c.R, c.width)
        for l in pc.plan(c.C, c.R, c.width, c.n, len(c.heads)):
            k = pc.instance(l)
            if k:
                cov.setdefault(k, set()).update(pc.edges(g, l))
    return cov


def test_every_reachable_instance_has_a_case_with_its_tile_edges():
    sw = pc.sweep()
    compiled = pc.compiled_instances()
    assert len(compiled) == 46 and len(UNREACHABLE) == 7 and UNREACHABLE < compiled
    assert set(sw) == compiled - UNREACHABLE and len(sw) == 39  # the reachable set is exactly what the mirror says
    cov = _coverage()
    for k in sorted(sw, key=str):
        assert k in cov, f"no case runs {k}"
    left = {}
    for k, es in sw.items():
        for e, r in es.items():  # which edges an instance's geometry allows is the sweep's answer, not a hand list
            if e not in cov[k]:
                assert r > R_CASE_MAX, f"{k}: no case with a '{e}' grid (the sweep shows one from R = {r})"
                left[(k, e)] = r
    assert left == EDGES_NOT_COVERED
    assert all(c.R <= R_CASE_MAX and (c.n <= 3 or c.tag == "sum260") for c in CASES + MIXED)


def test_stride_pool_image_and_head_variety():
    geo = {c.tag: pc.pred_geo(c.C, c.R, c.width) for c in CASES}
    assert {32, 33, 64, 65} <= {c.R for c in CASES}  # the pool switches on above 32, the stem's stride above 64
    odd_pool = [g for g in geo.values() if g.pool and g.h1 % 2]
    assert {g.s1 for g in odd_pool} == {1, 2}  # the uncovered row and column, behind either stem (tiled and workspace run every case)
    assert any(pc.pred_geo(c.C, c.R, pc.head_width(c, c.heads[0])).pool and c.R % 2 == 0 for c in MIXED)
    for L in (1, 3, 5):  # odd hin at stride 2, every such layer
        assert any(pc.tile_layer(g, L).hin % 2 for g in geo.values()), L
        assert any(pc.tile_layer(g, L).hin % 2 == 0 for g in geo.values()), L
    assert any(g.s1 == 2 and g.r % 2 for g in geo.values()) and any(g.s1 == 2 and g.r % 2 == 0 for g in geo.values())
    assert {c.C for c in CASES} == {1, 3, 4}
    assert {len(c.heads) for c in CASES} >= {1, 4}
    heads = [h for c in CASES for h in c.heads]
    assert {h.ctx for h in heads} >= {0, 1, 4}
    assert {h.kind for h in heads} == {pc.NORMAL, pc.CATEGORICAL, pc.BERNOULLI}
    assert any(h.tanh_loc for h in heads) and any(h.std_fixed > 0 for h in heads) and any(h.nout == pc.MAX_OUT for h in heads)
    assert any(len({h.kind for h in c.heads}) == 3 and len(c.heads) == 4 for c in CASES)
    assert any(c.n * len(c.heads) > 256 for c in CASES)  # pred_sum_kernel's strided partials
    for c in MIXED:
        assert len({pc.head_width(c, h) for h in c.heads}) > 1
    assert any(pc.fused_ok(c.C, c.R, [pc.head_width(c, h) for h in c.heads]) for c in MIXED)
    fused = [c.tag for c in CASES if pc.fused_ok(c.C, c.R, [c.width] * len(c.heads))]
    assert len(fused) >= 6 and {pc.by_tag(t).C for t in fused} == {1, 3, 4}, fused


# ------------------------------------------------------------------------------------------------- references
_SMALL = [c for c in CASES + MIXED if c.R <= 66 and c.n <= 3]


def _inputs(case):
    return ref.make_inputs(case)


@pytest.mark.parametrize("case", _SMALL, ids=lambda c: c.tag)
def test_chained_local_references_are_the_network_autograd_gives(case, monkeypatch):
    # the kernel's two likelihood constants are f32; torch.distributions has them in f64: compare at f64 round-off with the exact ones
    monkeypatch.setattr(ref, "HALF_LOG_2PI", 0.5 * math.log(2 * math.pi))
    monkeypatch.setattr(ref, "LOGIT_MAX", math.log1p(-ref.EPS32) - math.log(ref.EPS32))
    I = _inputs(case)
    placement = "tiled" if len({H.width for H in I.heads}) == 1 else "workspace"
    stored, dx = ref.simulate(case, I, placement, round32=False)
    x = I.x.double().requires_grad_(True)
    total, outs = ref.network_nll(case, I, x)
    (gx,) = torch.autograd.grad(ref.COEF * total, x)
    for S, o in zip(stored, outs):
        assert (S.outs - o).abs().max() <= 1e-12 * max(1.0, float(o.abs().max()))
    mine = sum(float(S.terms.sum()) for S in stored)
    assert abs(mine - float(total)) <= 1e-12 * max(1.0, abs(float(total)))
    assert (dx - gx).abs().max() <= 1e-12 * max(float(gx.abs().max()), 1e-30)
    assert float(gx.abs().max()) > 0


def test_planted_structure_is_there():
    for case in CASES:
        I = _inputs(case)
        stored, _ = ref.simulate(case, I, "tiled")
        g = pc.pred_geo(case.C, case.R, case.width)
        sat_imgs = None
        for hi, (H, S) in enumerate(zip(I.heads, stored)):
            a1 = S.fwd["a1"]
            assert int((a1[case.n - 1, :2] == 0).sum()) >= 2, case.tag  # pre-activation exactly 0 under the zero patch
            assert float(S.bwd["a1"][case.n - 1, :2][a1[case.n - 1, :2] == 0].abs().max()) > 0 or hi == I.hot, case.tag
            if g.pool:
                win = ref.pool_windows(a1, g.p)
                tied = (win == win[..., :1]).all(-1)
                assert int(tied[0].sum()) >= 4 * case.width / 2, case.tag  # whole windows tie under the flat patch
            _, _, _, _, branch, margin = ref.nll(H.head, S.outs, H.obs)
            assert float(margin.min()) > 1e-3, (case.tag, hi)  # no categorical pk near a clamp
            if hi == I.hot:
                assert all(b in ("sat", "clamped") for b in branch), (case.tag, branch)
                assert float(S.bwd["a6"].abs().max()) == 0
            elif H.head.kind != pc.NORMAL:
                assert all(b in ("free", "inside") for b in branch), (case.tag, hi, branch)
            r = ref.backward_refs(case, I, hi, S, "tiled")
            assert r["hid_margin"] > ref.HID_MARGIN_MIN, (case.tag, hi, r["hid_margin"])  # fc0's mask is decided
        if len(case.heads) > 1 and any(h.kind != pc.NORMAL for h in case.heads):
            assert I.hot is not None and any(float(S.bwd["a1"].abs().max()) > 0 for S in stored)


def test_pred_nll_branch_points_are_exact_and_take_the_stated_branch():
    seen = set()
    for case, pts in ref.nll_cases():
        I = ref.make_nll_inputs(case, pts)
        stored, _ = ref.simulate(case, I, "tiled")
        for H, S, (h, outs, obs, want) in zip(I.heads, stored, pts):
            assert float(S.fwd["a6"].abs().max()) == 0
            assert torch.equal(S.outs.float(), H.exact_outs.expand(2, -1)), outs  # the outputs are the chosen f32 values, exactly
            term, d, M, Md, branch, margin = ref.nll(h, S.outs, H.obs)
            assert branch == [want, want], (outs, branch)
            assert float(margin.min()) > 0.5
            seen.add((h.kind, want))
            if want in ("sat", "clamped"):
                assert float(d.abs().max()) == 0 and float(S.bwd["a6"].abs().max()) == 0
            else:
                assert float(S.bwd["a6"].abs().max()) > 0
            if h.kind == pc.CATEGORICAL and want == "free":  # tied obs rows: the first maximum
                k = [row.index(max(row)) for row in obs]
                p = torch.softmax(S.outs, 1)
                for b in range(2):
                    assert abs(float(d[b, k[b]] - (p[b, k[b]] - 1))) < 1e-15
    assert seen == {(pc.NORMAL, "softplus"), (pc.NORMAL, "linear"), (pc.NORMAL, "fixed"), (pc.BERNOULLI, "inside"), (pc.BERNOULLI, "clamped"),
                    (pc.CATEGORICAL, "sat"), (pc.CATEGORICAL, "free")}
    # the likelihoods agree with torch.distributions where no clamp of the kernel's own acts (f64)
    from predictor_ref import bernoulli_nll, categorical_nll, normal_nll

    for h, outs, obs, want in ref.NLL_POINTS:
        o, v = torch.tensor([outs], dtype=torch.float32).double().requires_grad_(True), torch.tensor(obs[:1], dtype=torch.float32).double()
        if h.kind == pc.NORMAL:
            t = normal_nll(o, v, bool(h.tanh_loc), h.std_fixed)
        elif h.kind == pc.CATEGORICAL:
            t = categorical_nll(o, v)
        else:
            t = bernoulli_nll(o, v)
        term, d, M, Md, _, _ = ref.nll(h, o.detach(), v)
        (gd,) = torch.autograd.grad(t, o)
        assert abs(float(term[0] - t)) <= 1e-7 * float(M[0]), (outs, float(term[0]), float(t))  # (HALF_LOG_2PI and LOGIT_MAX are f32 constants)
        if want not in ("clamped",):
            assert float((d[0] - gd[0]).abs().max()) <= 1e-7 * max(1.0, float(Md.max())), (outs, d, gd)


def test_recorded_constants_cover_a_fresh_measurement():
    cases = [(c, _inputs(c)) for c in CASES if c.R <= 35 and c.n <= 3] + [(c, ref.make_nll_inputs(c, p)) for c, p in ref.nll_cases()]
    w = ref.measure(cases)
    for fam, k in ref.K_ACC.items():
        assert ref.K_MARGIN * w[fam] <= k, (fam, w[fam], k)
    assert ref.K_MARGIN * w["nll"] <= ref.K_NLL, w["nll"]


# ------------------------------------------------------------------------------------------------- mutants
FAMILIES_OF = {  # mutant -> the site families it must apply to in at least one case ('ws:' = on the workspace placement)
    "corner_tap": {"a1", "a2", "g", "dx"}, "halo_replicate": {"a1", "a2", "g", "dx"}, "tile_row": {"a1", "a2", "g", "dx"},
    "tile_col": {"a1", "a2", "g", "dx"}, "group_channel": {"a1", "a2", "g"}, "last_chunk": {"a1", "a2", "g", "dx"},
    "parity": {"a1", "a2", "g", "dx"}, "pool_last_max": {"pool_bwd", "ws:pool_bwd"}, "odd_not_zeroed": {"pool_bwd", "ws:pool_bwd"},
    "lrelu_zero_side": {"g", "pool_bwd"}, "no_bias": {"a1", "a2", "outs"}, "mean_h6": {"outs"}, "last_ctx": {"outs"}, "last_head": {"dx"},
    "no_coef": {"a6"}, "saturated_contributes": {"a6"},
}


def _family(site, pooled_a1):
    if site == "a1":
        return "a1"
    if site in ("a2", "a3", "a4", "a5", "a6"):
        return "a2"
    return site


def _apply_mutant(case, I, placement, stored, mutant, applied):
    """Every site of every head: where the mutated reference differs from the reference at all, it differs by more than twice
    the tolerance somewhere (so nothing within the tolerance of one is within the tolerance of the other)."""
    pre = "ws:" if placement == "workspace" else ""
    g0 = pc.pred_geo(case.C, case.R, I.heads[0].width)
    parts, mparts = [], []
    for hi, S in enumerate(stored):
        for fn, kind in ((ref.forward_refs, "f"), (ref.backward_refs, "b")):
            base = fn(case, I, hi, S, placement)
            mut = fn(case, I, hi, S, placement, mutant) if mutant != "last_head" else {}
            if kind == "b":
                parts.append(base["dx1"])
                mparts.append(mut.get("dx1", base["dx1"]))
            for site, val in mut.items():
                if site in ("hid_margin", "dx1"):
                    continue
                mref = val[0]
                bref, tol = base[site]
                if torch.equal(mref, bref):
                    continue
                worst = float(((mref - bref).abs() / tol.clamp_min(1e-300)).max())
                assert worst > 2, (case.tag, placement, mutant, hi, site, worst)
                if kind == "f":
                    fam = "outs" if site == "outs" else "ap" if site == "ap" else _family(site, False)
                else:
                    fam = "a6" if site == "a6" else "ap" if site == "ap" else "pool_bwd" if (site == "a1" and g0.pool) else "g"
                applied.add(pre + fam)
    bref, tol = ref.dx_ref(parts)
    mref, _ = ref.dx_ref(mparts, drop_last=mutant == "last_head" and len(parts) > 1)
    if not torch.equal(mref, bref):
        worst = float(((mref - bref).abs() / tol).max())
        assert worst > 2, (case.tag, placement, mutant, "dx", worst)
        applied.add(pre + "dx")


_STORED = {}


def _stored(case, placement):
    key = (case.tag, placement)
    if key not in _STORED:
        I = _inputs(case)
        _STORED[key] = (I, ref.simulate(case, I, placement)[0])
    return _STORED[key]


_MUT_CASES = [c for c in CASES if c.R <= 66 and c.n <= 3]


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_mutant_is_told_from_the_reference(mutant):
    applied = set()
    for case in _MUT_CASES:
        I, stored = _stored(case, "tiled")
        _apply_mutant(case, I, "tiled", stored, mutant, applied)
    for case in [pc.by_tag("r35w24"), pc.by_tag("r50w16"), pc.by_tag("mixed_r40")]:  # the workspace placement: ap is a site of its own
        I, stored = _stored(case, "workspace")
        _apply_mutant(case, I, "workspace", stored, mutant, applied)
    assert FAMILIES_OF[mutant] <= applied, (mutant, sorted(FAMILIES_OF[mutant] - applied))
