"""cgen_conv2d_wgrad's generic kernel (wgrad_kernel<T, NTC>, kind 0) and tiled kernel (wgrad_tile_kernel<NCF, NJW, KS>, kind 1; through
the batch entry wgrad_tile_mega_kernel) called through the C ABI on every case of tests/wgrad_cases.py: cgen_conv2d_wgrad_plan_record,
cgen_conv2d_wgrad, cgen_wgrad_reduce, against the f64 reference and the tolerance of tests/wgrad_ref.py (its docstring derives every
term; the accumulation term is measured on the CPU from a sequential f32 chain, tests/test_wgrad_cases.py keeps the record).

Per case: the plan record equals the Python mirror before anything is launched; every element of grad_w and grad_b is finite and meets
the bound (no exclusions); every element of the split-K partials is written over its NaN prefill; the guard bands around the partials
and the gradients and the whole of every input parent keep their bits; a second call gives the bits of the first.

Layout: every input view lies in a parent that is NaN wherever the view is not -- other samples, rows, columns (the odd pixels of the
strided view) and channels; only the channels [c, cpad) of a view that declares cpad hold zeros.  Anything a kernel lets in from outside
a view makes a gradient NaN."""
import ctypes as C
import time

import pytest
import torch

import wgrad_cases as T
import wgrad_ref as R
from gpu_views import _bits, cv

pytestmark = pytest.mark.gpu
GUARD = 1 << 14  # floats on each side of every contiguous output (64 KiB), filled with random finite values and compared bit for bit
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    from causal_gen_amd import _lib

    return _lib.require_gpu()


def _place(case, c, vw, values, tdt):
    """(parent, view) of `values` [n, h, w, c] laid out by `vw`; the view's picture in the mirror is the real one."""
    n, h, w = case.n, case.h, case.w
    parent = torch.full(T.parent_shape(case, c, vw), NAN, dtype=tdt, device="cuda")
    assert parent.data_ptr() % 256 == 0
    region = parent[:n] if vw.bcast else parent[:n, :vw.step * h:vw.step, :vw.step * w:vw.step]
    region[..., vw.off:vw.off + c] = (values[:, :1, :1] if vw.bcast else values).to(tdt).cuda()
    if vw.cpad > c:
        region[..., vw.off + c:vw.off + vw.cpad] = 0
    v = region[..., vw.off:vw.off + c]
    if vw.bcast:
        v = v.expand(n, h, w, c)
    view = cv(v, vw.cpad)
    m = T.view(case, c, vw)
    assert (view.p % 256, view.sn, view.sh, view.sw, view.c, view.cpad) == (m["p"], m["sn"], m["sh"], m["sw"], m["c"], m["cpad"])
    return parent, view


def _guarded(count, values=None):
    """A contiguous f32 buffer of `count` elements (NaN, or `values`) between two guard bands of random finite values."""
    buf = torch.randn((count + 2 * GUARD,), device="cuda")
    buf[GUARD:GUARD + count] = NAN if values is None else values.reshape(-1).float().cuda()
    return buf, buf[GUARD:GUARD + count]


def _bands(buf):
    return torch.cat([_bits(buf[:GUARD]), _bits(buf[-GUARD:])])


class Run:
    """The parents, views, partials and arguments of one case."""

    def __init__(self, lib, case, I):
        from causal_gen_amd import _lib

        self.lib, self.case, self.I = lib, case, I
        a = self.args = _lib.WgradArgs()
        a.dtype = _lib.F32 if case.dt == "f32" else _lib.F16
        a.n, a.h, a.w, a.ks, a.nseg, a.act = case.n, case.h, case.w, case.ks, len(case.segs), case.act
        self.inputs = []
        for s, c in enumerate(case.segs):
            parent, a.seg[s] = _place(case, c, case.v(s), I.segs[s], I.tdt)
            self.inputs.append(parent)
        parent, a.gout = _place(case, case.co, case.gv, I.g, I.tdt)
        self.inputs.append(parent)
        self.inputs_before = [p.clone() for p in self.inputs]
        self.ci, self.taps = sum(case.segs), case.ks * case.ks
        self.nw = case.co * self.taps * self.ci
        # the plan, with the bias partial named as the launch will see it
        a.partial_w = 256
        a.partial_b = 256 if case.bias else None
        rec = (C.c_int32 * T.REC_INTS)(*([-1] * T.REC_INTS))
        self.nsplit = lib.conv2d_wgrad_plan_record(C.byref(a), rec)
        self.record = list(rec)
        a.nsplit = self.nsplit
        self.pw_buf, self.pw = _guarded(self.nsplit * self.nw)
        self.pb_buf, self.pb = _guarded(self.nsplit * case.co)
        a.partial_w = self.pw.data_ptr()
        a.partial_b = self.pb.data_ptr() if case.bias else None
        self.gw_buf, self.gw = _guarded(self.nw, I.prev_w)
        self.gb_buf, self.gb = _guarded(case.co, I.prev_b)
        self.gw0, self.gb0 = self.gw_buf.clone(), self.gb_buf.clone()
        self.pbands = [_bands(self.pw_buf).clone(), _bands(self.pb_buf).clone()]

    def wgrad(self):
        self.pw.fill_(NAN)
        self.pb.fill_(NAN)
        self.lib.conv2d_wgrad(C.byref(self.args), None)
        torch.cuda.synchronize()

    def reduce(self):
        from causal_gen_amd import _lib

        case = self.case
        self.gw_buf.copy_(self.gw0)
        self.gb_buf.copy_(self.gb0)
        d = _lib.WredDesc()
        d.partial_w, d.partial_b = self.pw.data_ptr(), (self.pb.data_ptr() if case.bias else None)
        d.grad_w, d.grad_b = self.gw.data_ptr(), (self.gb.data_ptr() if case.bias else None)
        d.co, d.ci_total, d.ks, d.nsplit = case.co, self.ci, case.ks, self.nsplit
        d.accumulate, d.unscale, d.layout = int(case.accumulate), case.unscale, 0
        d.numel = self.nw + case.co
        nch = -(-d.numel // 1024)
        self.keep = (torch.frombuffer(bytearray(bytes(d)), dtype=torch.uint8).cuda(), torch.zeros(nch, dtype=torch.int32, device="cuda"),
                     torch.arange(nch, dtype=torch.int32, device="cuda"))
        self.lib.wgrad_reduce(self.keep[0].data_ptr(), self.keep[1].data_ptr(), self.keep[2].data_ptr(), nch, None)
        torch.cuda.synchronize()

    def check_partials(self):
        """Every partial element is written, nothing around them and nothing of the inputs is touched."""
        case = self.case
        assert not bool(torch.isnan(self.pw).any()), f"{int(torch.isnan(self.pw).sum())} of {self.pw.numel()} elements of partial_w were never written"
        if case.bias:
            assert not bool(torch.isnan(self.pb).any()), "elements of partial_b were never written"
        else:
            assert bool(torch.isnan(self.pb).all()), "partial_b was written without being passed"
        for buf, was in zip((self.pw_buf, self.pb_buf), self.pbands):
            assert torch.equal(_bands(buf), was), "a write outside the partials"
        for p, before in zip(self.inputs, self.inputs_before):
            assert torch.equal(_bits(p), _bits(before)), "an input parent changed"

    def check(self, ref):
        """The bound on grad_w and grad_b and the guard bands around them.  Returns the worst err / tol of both."""
        case = self.case
        for buf, was in ((self.gw_buf, self.gw0), (self.gb_buf, self.gb0)):
            assert torch.equal(_bands(buf), _bands(was)), "a write outside the gradient"
        gw = self.gw.cpu().view(case.co, self.ci, case.ks, case.ks)  # (the reduce writes OIHW)
        assert bool(torch.isfinite(gw).all()), f"{int((~torch.isfinite(gw)).sum())} elements of grad_w are not finite: something from outside a view came in"
        err = (gw.double() - ref.w).abs()
        worst_w = float((err / ref.tol_w.clamp_min(1e-300)).max())
        worst_b = 0.0
        if case.bias:
            gb = self.gb.cpu()
            assert bool(torch.isfinite(gb).all())
            eb = (gb.double() - ref.b).abs()
            worst_b = float((eb / ref.tol_b.clamp_min(1e-300)).max())
        else:
            assert torch.equal(_bits(self.gb_buf), _bits(self.gb0)), "grad_b was written without being passed"
        print(f"wgrad_f64 {T.family(case)} {case.id()} worst err/tol w {worst_w:.3f} b {worst_b:.3f} (k {ref.k:g})")
        bad = ~(err <= ref.tol_w)
        assert not bad.any(), (f"grad_w: {int(bad.sum())} of {bad.numel()} outside the k={ref.k} bound; worst err/tol {worst_w:.3g}; first at "
                               f"(co, ci, dy, dx) = {tuple(int(v) for v in bad.nonzero()[0])}")
        if case.bias:
            assert bool((eb <= ref.tol_b).all()), f"grad_b outside the k={ref.k} bound; worst err/tol {worst_b:.3g}"
        return max(worst_w, worst_b)


def _env(monkeypatch, case):
    if case.generic:
        monkeypatch.setenv("CGEN_WGRAD_GENERIC", "1")
    else:
        monkeypatch.delenv("CGEN_WGRAD_GENERIC", raising=False)


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id())
def test_wgrad_against_f64(lib, case, monkeypatch):
    t0 = time.time()
    I = R.make_inputs(case, lib.h16_is_bf16)  # (on the CPU, before anything runs on the GPU)
    plan = T.plan(T.problem(case))
    ref = R.reference(case, I, plan)
    assert ref.flag_share <= R.FLAG_SHARE_MAX
    _env(monkeypatch, case)
    run = Run(lib, case, I)
    assert run.record == T.record(T.problem(case)), "cgen_conv2d_wgrad_plan_record differs from the mirror"
    assert T.tag(plan) == case.want
    run.wgrad()
    run.check_partials()
    first = (_bits(run.pw).clone(), _bits(run.pb).clone())
    run.reduce()
    run.check(ref)
    grads = (_bits(run.gw_buf).clone(), _bits(run.gb_buf).clone())
    run.wgrad()
    run.check_partials()
    assert torch.equal(first[0], _bits(run.pw)) and torch.equal(first[1], _bits(run.pb)), "a second call gives other partials"
    run.reduce()
    assert torch.equal(grads[0], _bits(run.gw_buf)) and torch.equal(grads[1], _bits(run.gb_buf)), "a second reduce gives other bits"
    print(f"wgrad_f64 {case.id()} took {time.time() - t0:.2f} s")


def test_tiled_kernel_through_the_batch_entry(lib, monkeypatch):
    """One cgen_conv2d_wgrad_batch_plan over every kind-1 case, two streaming cases and one f32 case: eligible 1 / 1 / 0, two launches (the
    all-variant tiled kernel and the streaming kernel); uncapped and with eight resident workgroups the slabs equal the single launches
    bit for bit, twice in a row."""
    from causal_gen_amd import _lib

    monkeypatch.delenv("CGEN_WGRAD_GENERIC", raising=False)
    tiled = [c for c in T.CASES if T.plan(T.problem(c))["kind"] == 1]
    stream = [T.Case("h16", 2, 12, 12, (24,), 32, 3, T.RELU, want="stream"), T.Case("h16", 2, 12, 12, (32, 4), 8, 3, T.GELU, (T.AL, T.pad8(4)), want="stream")]
    cases = tiled + stream + [next(c for c in T.CASES if c.dt == "f32")]
    assert len(tiled) >= 18 and {T.plan(T.problem(c))["kind"] for c in stream} == {2, 3}
    runs, singles = [], []
    for c in cases:
        run = Run(lib, c, R.make_inputs(c, lib.h16_is_bf16))
        run.wgrad()
        singles.append((_bits(run.pw).clone(), _bits(run.pb).clone()))
        runs.append(run)
    n = len(runs)
    arr = (_lib.WgradArgs * n)(*[r.args for r in runs])
    nbytes, nl = C.c_int64(0), C.c_int32(0)
    elig = (C.c_int32 * n)()
    lib.conv2d_wgrad_batch_plan(arr, n, None, 0, C.byref(nbytes), None, 0, C.byref(nl), elig)
    host = (C.c_char * max(nbytes.value, 1))()
    launches = (_lib.WgradBatchLaunch * max(nl.value, 1))()
    lib.conv2d_wgrad_batch_plan(arr, n, host, nbytes.value, C.byref(nbytes), launches, nl.value, C.byref(nl), elig)
    assert list(elig) == [1] * len(tiled) + [1] * len(stream) + [0]
    assert nl.value == 2 and sorted(launches[i].ncf for i in range(2)) == [-3, 0]
    blob = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).cuda()
    for cap in (0, 8):
        for rep in range(2):
            for r in runs[:-1]:
                r.pw.fill_(NAN)
                r.pb.fill_(NAN)
            lib.conv2d_wgrad_batch_run(blob.data_ptr(), launches, nl.value, cap, None)
            torch.cuda.synchronize()
            for r, (pw, pb) in list(zip(runs, singles))[:-1]:
                r.check_partials()
                assert torch.equal(_bits(r.pw), pw) and torch.equal(_bits(r.pb), pb), ("packed launch != single launch", cap, rep, r.case.id())
