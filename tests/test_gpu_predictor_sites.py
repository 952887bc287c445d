"""csrc/predictor.hip on the MI355X, site by site: every activation plane the tiled and workspace placements leave in the workspace
after a forward call, every gradient plane after a backward call, outs, terms, loss and dx, each element against the f64 reference
of that one layer computed from the planes the device itself stored (tests/predictor_site_ref.py), for the cases of
tests/predictor_cases.py (every reachable tiled instance, tests/test_predictor_cases.py proves it).  Output buffers start as NaN
between random guard bands that are compared bit for bit; inputs are compared whole after the calls.  The fused placement, whose
stack lives in LDS, is held to the workspace placement's bits and to the same references.  No element is left out."""
import ctypes
import math

import pytest
import torch

import predictor_cases as pc
import predictor_site_ref as ref
from gpu_views import _bits
from predictor_cases import CASES, MIXED

pytestmark = pytest.mark.gpu

GUARD = 64  # floats on either side of an output (256 bytes: the output keeps its alignment)
WORST = {}  # (placement, family) -> (worst err / tol, case): printed as evidence, no bound comes from it
_INPUTS = {}


def _all_cases():
    return [(c, None) for c in CASES + MIXED] + ref.nll_cases()


def _inputs(case, pts):
    if case.tag not in _INPUTS:
        _INPUTS[case.tag] = ref.make_nll_inputs(case, pts) if pts else ref.make_inputs(case)
    return _INPUTS[case.tag]


class Out:
    """A NaN-filled f32 destination of `count` floats between two random finite guard bands."""

    def __init__(self, count, seed):
        g = torch.Generator().manual_seed(seed)
        whole = torch.full((count + 2 * GUARD,), float("nan"))
        whole[:GUARD] = torch.randn(GUARD, generator=g)
        whole[GUARD + count:] = torch.randn(GUARD, generator=g)
        self.whole = whole.cuda()
        self.v = self.whole[GUARD:GUARD + count]
        self.before = self.whole.clone()
        self.count = count
        assert self.v.data_ptr() % 256 == 0

    def ptr(self):
        return self.v.data_ptr()

    def check_guards(self, what):
        w, b = _bits(self.whole), _bits(self.before)
        assert torch.equal(w[:GUARD], b[:GUARD]) and torch.equal(w[GUARD + self.count:], b[GUARD + self.count:]), f"{what}: a write outside the buffer"

    def refill(self):
        self.whole.copy_(self.before)


class Device:
    """The inputs of a case on the GPU, the head records over them, and copies to compare with after the calls."""

    def __init__(self, case, I):
        from causal_gen_amd import _lib

        self.case, self.I = case, I
        self.x = I.x.cuda()
        self.coef = I.coef.cuda()
        self.keep = [self.x, self.coef]
        self.recs = []
        for H in I.heads:
            h = H.head
            r = _lib.PredHead()
            r.c, r.res, r.width, r.nout, r.ctx, r.kind, r.tanh_loc = case.C, case.R, H.width, h.nout, h.ctx, h.kind, h.tanh_loc
            r.std_fixed = h.std_fixed
            for i in range(8):
                wt, bt = H.w[i].contiguous().cuda(), H.b[i].contiguous().cuda()
                self.keep += [wt, bt]
                r.w[i], r.b[i] = wt.data_ptr(), bt.data_ptr()
            obs = H.obs.contiguous().cuda()
            self.keep.append(obs)
            r.obs, r.obs_stride = obs.data_ptr(), obs.shape[1]
            if H.y is not None:
                y = H.y.contiguous().cuda()
                self.keep.append(y)
                r.y = y.data_ptr()
            self.recs.append(r)
        self.copies = [t.clone() for t in self.keep]

    def records(self, idx):
        from causal_gen_amd import _lib

        return (_lib.PredHead * len(idx))(*[self.recs[i] for i in idx])

    def check_inputs(self):
        for t, c in zip(self.keep, self.copies):
            assert torch.equal(_bits(t), _bits(c)), "an input was written"


def _note(placement, fam, ratio, tag):
    key = (placement, fam)
    if ratio > WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (ratio, tag)


def _check(case, placement, hi, site, fam, got, want, tol):
    got, want, tol = got.double(), want.double(), tol.double()
    assert got.shape == want.shape, (case.tag, site, got.shape, want.shape)
    err = (got - want).abs()
    bad = ~(err <= tol)  # (a NaN -- an element never written -- is bad)
    ratio = float((err / tol.clamp_min(1e-300)).nan_to_num(nan=math.inf).max()) if err.numel() else 0.0
    _note(placement, fam, ratio, case.tag)
    print(f"SITE {case.tag:10s} {placement:9s} head {hi} {site:6s} worst err/tol {ratio:.3f}")
    assert not bad.any(), (f"{case.tag} {placement} head {hi} {site}: {int(bad.sum())} of {bad.numel()} outside the bound, worst err/tol "
                           f"{ratio:.3g}, first at {bad.nonzero()[0].tolist()}: got {got[bad][:3].tolist()} want {want[bad][:3].tolist()}")


FAMILY = {"a1": "stem", "ap": "pool", "a2": "fwd3", "a3": "fwd3", "a4": "fwd3", "a5": "fwd3", "a6": "fwd3", "outs": "tail", "terms": "nll"}
BFAMILY = {"a6": "tail_bwd", "a5": "bwd3", "a4": "bwd3", "a3": "bwd3", "a2": "bwd3", "a1": "bwd3", "ap": "bwd3"}


def _planes(flat, g, n, stride, base, with_ap):
    """The planes of one head's stacks in a host copy of the workspace: name -> [n, ch, h, h] (f64 of the stored f32)."""
    w = g.w
    shapes = {"a1": (g.a1, w, g.h1), "a2": (g.a2, 2 * w, g.h2), "a3": (g.a3, 2 * w, g.h2), "a4": (g.a4, 4 * w, g.h4), "a5": (g.a5, 4 * w, g.h4),
              "a6": (g.a6, 8 * w, g.h6)}
    if with_ap and g.pool:
        shapes["ap"] = (g.ap, w, g.p)
    out = {}
    for name, (off, ch, h) in shapes.items():
        out[name] = torch.stack([flat[base + b * stride + off: base + b * stride + off + ch * h * h].view(ch, h, h) for b in range(n)]).double()
    return out


def _untouched(flat, before, lo, hi, what):
    assert torch.equal(_bits(flat[lo:hi]), _bits(before[lo:hi])), f"{what}: written"


def _check_forward(case, I, placement, hi, S):
    r = ref.forward_refs(case, I, hi, S, placement)
    for site, (want, tol) in r.items():
        got = S.outs if site == "outs" else S.terms if site == "terms" else S.fwd[site]
        _check(case, placement, hi, site, FAMILY[site], got, want, tol)
    H = I.heads[hi]
    if hasattr(H, "exact_outs"):  # pred_nll's branch points: the outputs are the chosen values, bit for bit
        assert torch.equal(S.outs.float(), H.exact_outs.expand(case.n, -1)), (case.tag, hi, S.outs)


def _check_backward(case, I, placement, hi, S):
    r = ref.backward_refs(case, I, hi, S, placement)
    assert r["hid_margin"] > 1, (case.tag, hi, r["hid_margin"])  # fc0's mask, taken from the f64 hid, is decided
    for site in ("a6", "a5", "a4", "a3", "a2", "ap", "a1"):
        if site in r:
            _check(case, placement, hi, site + "'", BFAMILY[site], S.bwd[site], r[site][0], r[site][1])
    return r["dx1"]


def _loss_check(case, placement, terms, loss):
    t = terms.double()
    k = (t.numel() + 255) // 256 + 8 + 1  # pred_sum_kernel: a strided partial per thread, then a tree of 8 levels; every add rounds once
    _check(case, placement, "-", "loss", "sum", loss.double(), t.sum().view(1), (k * ref.U32 * t.abs().sum() + ref.TINY).view(1))


def _same_bits(a, b):
    """Positions where two f32 tensors differ in bits, the sign of zero aside."""
    return (_bits(a) != _bits(b)) & ~((a == 0) & (b == 0))


@pytest.mark.parametrize("case,pts", [(c, p) for c, p in _all_cases() if c not in MIXED], ids=lambda v: v.tag if isinstance(v, pc.Case) else "")
def test_tiled_every_site_within_its_bound(case, pts):
    from causal_gen_amd import _lib

    lib = _lib.require_gpu()
    I = _inputs(case, pts)
    D = Device(case, I)
    n, nh = case.n, len(case.heads)
    g = pc.pred_geo(case.C, case.R, case.width)
    recs = D.records(range(nh))
    need = _lib.i64(0)
    lib.predictor_tiled_workspace(recs, nh, n, ctypes.byref(need))
    assert need.value == n * nh * g.total
    ws, terms, outs, loss, dx = Out(need.value, 1), Out(n * nh, 2), Out(nh * n * pc.MAX_OUT, 3), Out(1, 4), Out(I.x.numel(), 5)
    st = torch.cuda.current_stream().cuda_stream
    lib.predictor_tiled_fwd(recs, nh, n, D.x.data_ptr(), ws.ptr(), need.value, terms.ptr(), outs.ptr(), loss.ptr(), st)
    torch.cuda.synchronize()
    for o, name in ((ws, "ws"), (terms, "terms"), (outs, "outs"), (loss, "loss")):
        o.check_guards(name)
    assert torch.equal(_bits(dx.whole), _bits(dx.before))  # the forward call does not touch dx
    fws, fterms, fouts, floss = ws.v.cpu(), terms.v.cpu().view(n, nh), outs.v.cpu().view(nh, n, pc.MAX_OUT), loss.v.cpu()
    before = ws.before[GUARD:GUARD + need.value].cpu()
    stored = []
    for hi, H in enumerate(I.heads):
        S = ref.Stored()
        S.fwd = _planes(fws, g, n, nh * g.total, hi * g.total, False)
        S.outs = fouts[hi, :, :H.head.nout].double()
        S.terms = fterms[:, hi].double()
        _check_forward(case, I, "tiled", hi, S)
        assert torch.isnan(fouts[hi, :, H.head.nout:]).all(), "outs beyond nout written"
        stored.append(S)
        for b in range(n):  # the tiled path pools while staging: ap and the rounding tail of every stack keep their prefill
            base = (b * nh + hi) * g.total
            _untouched(fws, before, base + g.ap, base + g.a2, f"{case.tag}: ap of stack ({b}, {hi})")
            _untouched(fws, before, base + g.used, base + g.total, f"{case.tag}: rounding tail of stack ({b}, {hi})")
    _loss_check(case, "tiled", fterms.reshape(-1), floss)
    # ---- backward (it recomputes the forward into ws)
    runs = []
    for rep in range(2):
        ws.refill()
        dx.refill()
        lib.predictor_tiled_bwd(recs, nh, n, D.x.data_ptr(), ws.ptr(), need.value, D.coef.data_ptr(), dx.ptr(), st)
        torch.cuda.synchronize()
        ws.check_guards("ws (backward)")
        dx.check_guards("dx")
        runs.append((ws.v.cpu(), dx.v.cpu()))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1])), "a second backward differs"
    bws, gdx = runs[0]
    parts = []
    for hi, S in enumerate(stored):
        S.bwd = _planes(bws, g, n, nh * g.total, hi * g.total, False)
        parts.append(_check_backward(case, I, "tiled", hi, S))
        for b in range(n):
            base = (b * nh + hi) * g.total
            _untouched(bws, before, base + g.ap, base + g.a2, f"{case.tag}: ap of stack ({b}, {hi}) after backward")
            _untouched(bws, before, base + g.used, base + g.total, f"{case.tag}: rounding tail of stack ({b}, {hi}) after backward")
    want, tol = ref.dx_ref(parts)
    _check(case, "tiled", "-", "dx", "stem_bwd", gdx.view(I.x.shape), want, tol)
    # the backward call writes neither terms, outs nor loss
    assert torch.equal(_bits(terms.v.cpu()), _bits(fterms.reshape(-1))) and torch.equal(_bits(outs.v.cpu()), _bits(fouts.reshape(-1)))
    assert torch.equal(_bits(loss.v.cpu()), _bits(floss))
    D.check_inputs()


_WS = {}  # case tag -> what the workspace placement gave (the fused test compares with it)


def _run_flat(lib, D, idx, n, use_ws):
    """cgen_predictor_fwd then cgen_predictor_bwd on the heads `idx`: host copies of ws after either call, terms, outs, loss, dx."""
    from causal_gen_amd import _lib

    nh = len(idx)
    recs = D.records(idx)
    per = _lib.i64(0)
    lib.predictor_workspace(recs, nh, ctypes.byref(per))
    ws = Out(n * per.value, 11) if use_ws else None
    terms, outs, loss, dx = Out(n * nh, 12), Out(nh * n * pc.MAX_OUT, 13), Out(1, 14), Out(D.x.numel(), 15)
    st = torch.cuda.current_stream().cuda_stream
    lib.predictor_fwd(recs, nh, n, D.x.data_ptr(), ws.ptr() if ws else None, terms.ptr(), outs.ptr(), loss.ptr(), st)
    torch.cuda.synchronize()
    fws = ws.v.cpu() if ws else None
    assert torch.equal(_bits(dx.whole), _bits(dx.before))
    if ws:
        ws.refill()
    lib.predictor_bwd(recs, nh, n, D.x.data_ptr(), ws.ptr() if ws else None, D.coef.data_ptr(), dx.ptr(), st)
    torch.cuda.synchronize()
    for o, name in ((terms, "terms"), (outs, "outs"), (loss, "loss"), (dx, "dx")) + (((ws, "ws"),) if ws else ()):
        o.check_guards(name)
    return dict(per=per.value, fws=fws, bws=ws.v.cpu() if ws else None, before=ws.before[GUARD:GUARD + ws.count].cpu() if ws else None,
                terms=terms.v.cpu().view(n, nh), outs=outs.v.cpu().view(nh, n, pc.MAX_OUT), loss=loss.v.cpu(), dx=dx.v.cpu().view(D.x.shape))


def _workspace(case, pts):
    """One head at a time (so that the stack survives), every site checked; then the multi-head call."""
    from causal_gen_amd import _lib

    if case.tag in _WS:
        return _WS[case.tag]
    lib = _lib.require_gpu()
    I = _inputs(case, pts)
    D = Device(case, I)
    n, nh = case.n, len(case.heads)
    singles, stored, parts = [], [], []
    for hi, H in enumerate(I.heads):
        g = pc.pred_geo(case.C, case.R, H.width)
        r = _run_flat(lib, D, [hi], n, True)
        assert r["per"] == g.total
        S = ref.Stored()
        S.fwd = _planes(r["fws"], g, n, g.total, 0, True)
        S.bwd = _planes(r["bws"], g, n, g.total, 0, True)
        S.outs = r["outs"][0, :, :H.head.nout].double()
        S.terms = r["terms"][:, 0].double()
        _check_forward(case, I, "workspace", hi, S)
        assert torch.isnan(r["outs"][0, :, H.head.nout:]).all(), "outs beyond nout written"
        _loss_check(case, "workspace", r["terms"].reshape(-1), r["loss"])
        parts.append(_check_backward(case, I, "workspace", hi, S))
        want, tol = ref.dx_ref(parts[-1:])
        _check(case, "workspace", hi, "dx", "stem_bwd", r["dx"], want, tol)
        for b in range(n):
            for w in (r["fws"], r["bws"]):
                _untouched(w, r["before"], b * g.total + g.used, (b + 1) * g.total, f"{case.tag}: rounding tail of stack {b}")
        singles.append(r)
        stored.append(S)
    multi = _run_flat(lib, D, list(range(nh)), n, True)
    for hi, H in enumerate(I.heads):
        assert torch.equal(_bits(multi["terms"][:, hi]), _bits(singles[hi]["terms"][:, 0])), (case.tag, hi, "terms differ from the single-head call")
        assert torch.equal(_bits(multi["outs"][hi]), _bits(singles[hi]["outs"][0])), (case.tag, hi, "outs differ from the single-head call")
    acc = singles[0]["dx"].clone()
    for r in singles[1:]:
        acc = acc + r["dx"]  # f32, in head order: what the owning thread does
    diff = _same_bits(multi["dx"], acc)
    assert not diff.any(), (case.tag, "dx is not the f32 sum of the single-head calls in head order", diff.nonzero()[:4].tolist())
    want, tol = ref.dx_ref(parts)
    _check(case, "workspace", "-", "dx", "stem_bwd", multi["dx"], want, tol)
    _loss_check(case, "workspace", multi["terms"].reshape(-1), multi["loss"])
    D.check_inputs()
    _WS[case.tag] = dict(D=D, I=I, multi=multi, stored=stored, parts=parts)
    return _WS[case.tag]


_WS_CASES = [(c, p) for c, p in _all_cases() if c.n <= 3]


@pytest.mark.parametrize("case,pts", _WS_CASES, ids=lambda v: v.tag if isinstance(v, pc.Case) else "")
def test_workspace_every_site_within_its_bound(case, pts):
    _workspace(case, pts)


_FUSED = [(c, p) for c, p in _WS_CASES if pc.fused_ok(c.C, c.R, [pc.head_width(c, h) for h in c.heads])]


@pytest.mark.parametrize("case,pts", _FUSED, ids=lambda v: v.tag if isinstance(v, pc.Case) else "")
def test_fused_gives_the_workspace_placements_bits(case, pts):
    from causal_gen_amd import _lib

    lib = _lib.require_gpu()
    W = _workspace(case, pts)
    D, I, n, nh = W["D"], W["I"], case.n, len(case.heads)
    assert lib._raw_cgen_predictor_supported(D.records(range(nh)), nh) == 1
    r = _run_flat(lib, D, list(range(nh)), n, False)
    for name in ("terms", "outs", "loss", "dx"):  # one template, the same arithmetic in the same order
        a, b = r[name], W["multi"][name]
        keep = ~(torch.isnan(a) & torch.isnan(b))  # (outs beyond nout: the prefill on both sides)
        diff = _same_bits(a, b) & keep
        assert not diff.any(), (case.tag, name, "fused differs from workspace", diff.nonzero()[:4].tolist())
    for hi, (H, S) in enumerate(zip(I.heads, W["stored"])):  # and the f64 bounds, from the planes the workspace placement stored
        fr = ref.forward_refs(case, I, hi, S, "workspace")
        _check(case, "fused", hi, "outs", "tail", r["outs"][hi, :, :H.head.nout], fr["outs"][0], fr["outs"][1])
        t, _, M, _, _, _ = ref.nll(H.head, r["outs"][hi, :, :H.head.nout].double(), H.obs)
        _check(case, "fused", hi, "terms", "nll", r["terms"][:, hi], t, ref.K_NLL * ref.U32 * M)
        assert torch.isnan(r["outs"][hi, :, H.head.nout:]).all()
    want, tol = ref.dx_ref(W["parts"])
    _check(case, "fused", "-", "dx", "stem_bwd", r["dx"], want, tol)
    D.check_inputs()


def test_plan_entry_reports_the_mirrors_record_for_every_case():
    from causal_gen_amd import _lib

    lib = _lib.require_gpu()
    for case, _ in _all_cases():
        if case in MIXED:
            continue
        nh = len(case.heads)
        recs = (_lib.PredHead * nh)()
        for r in recs:
            r.c, r.res, r.width, r.nout, r.kind, r.obs_stride = case.C, case.R, case.width, 2, _lib.PRED_NORMAL, 1
        rec = (_lib.i32 * (8 * 13))()
        count = _lib.i32(0)
        lib.predictor_tiled_plan(recs, nh, case.n, rec, 13, ctypes.byref(count))
        assert [tuple(rec[8 * i:8 * i + 8]) for i in range(count.value)] == [tuple(l) for l in pc.plan(case.C, case.R, case.width, case.n, nh)], case.tag


def test_zz_worst_ratios_for_the_record():
    """Evidence only: the worst err / tol per placement and family over the tests above (run after them in file order)."""
    for (placement, fam), (ratio, tag) in sorted(WORST.items()):
        print(f"WORST {placement:9s} {fam:9s} {ratio:.3f}  ({tag})")
