"""cgen_block3 called through the C ABI -- the weight images from cgen_weight_prep modes 2-7 (0 / 1 for the down Block's projection),
then ONE launch, no Engine -- on every case of tests/block_cases.py, against the two-stage f64 reference and the per-element bound of
tests/block_ref.py (its docstring derives every term; tests/test_block_cases.py keeps the CPU side: instance keys, reachability,
mutants, the measured accumulation constants).

Per case: cgen_block3_plan names the instance the table expects, before anything is launched; every element of the bottleneck meets
the stage-1 bound and every element of every output the stage-2 bound, computed from the bottleneck the kernel wrote; remainder planes
hold hi + rem to the bound with hi the nearest 16-bit value; nothing outside the output views changes; a second launch into fresh
parents gives the same bits.

Layout: every view lies in a parent that is NaN wherever the view is not (tests/gpu_views.Arena.place) -- other images, rows, columns
and channels; only the channels [c, 8) of the parents segment hold zeros, as cgen_view.cpad promises.  The kernels form no address
outside a view: halo pixels outside the image come from a 64-byte block of zeros (g_b3zero) or are written as zeros in LDS, every
load and store of csrc/block.hip is predicated on 0 <= y < H, 0 <= x < W and on the channel group lying below ceil8(c) -- so a parent
need not be larger than its view, and anything taken from outside a view shows as NaN in the result.  The biases are read in groups
of four floats below Co only; they and the weight images still get NaN behind their last value (320 floats, 64 KiB), so that a
fragment or a bias group fetched from past the end would show the same way."""
import ctypes

import pytest
import torch

import block_cases as T
import block_ref as R
from gpu_views import Arena, _bits, cv

pytestmark = pytest.mark.gpu
SLACK = 32768  # elements of NaN behind every weight image


@pytest.fixture(scope="module")
def lib():
    from causal_gen_amd import _lib

    return _lib.require_gpu()


def _ceil(v, m):
    return -(-v // m) * m


def image_descs(case, I):
    """role -> (OIHW source, dict of cgen_wprep_desc fields) of the weight images the case's launch reads."""
    b, co, ci = case.b, case.co, sum(case.segs)
    nks = (9 * b + 15) // 16
    w1 = dict(co=b, ci_total=ci, ks=3, seg_off=0, rows_pad=0)
    w2 = dict(co=co, ci_total=b, ks=3, seg_off=0, rows_pad=0, nseg=1, seg_c=[b])
    out = {}
    if case.dir == "fwd":
        nch = sum(_ceil(c, 32) // 32 for c in case.segs)
        out["w_a"] = (I.w1, dict(w1, mode=2, nseg=len(case.segs), seg_c=case.segs, k_pad=nch * 18, numel=_ceil(b, 32) // 32 * nch * 18 * 512))
        if case.a16:
            out["w_a16"] = (I.w1, dict(w1, mode=6, nseg=1, seg_c=case.segs, k_pad=case.segs[0] // 32, numel=9 * (case.segs[0] // 32) * 512))
        out["w0"] = (I.w2, dict(w2, mode=4, k_pad=nks, numel=_ceil(co, 32) // 32 * nks * 512))
        if case.down:
            krow = T.proj_krow(ci)
            out["w_proj"] = (I.wp, dict(co=co, ci_total=ci, ks=1, mode=0, nseg=1, seg_off=0, seg_c=[ci], rows_pad=_ceil(co, 16), k_pad=krow, numel=_ceil(co, 16) * krow))
    else:
        nch = _ceil(_ceil(co, 8), 32) // 32
        out["w_a"] = (I.w2, dict(w2, mode=3, k_pad=nch * 18, numel=_ceil(b, 32) // 32 * nch * 18 * 512))
        if case.a16:
            out["w_a16"] = (I.w2, dict(w2, mode=7, k_pad=co // 32, numel=9 * (co // 32) * 512))
        for j, k in enumerate(case.dsegs):
            c = case.segs[k]
            out[f"w{j}"] = (I.w1, dict(w1, mode=5, nseg=1, seg_off=case.seg_off(k), seg_c=[c], k_pad=nks, numel=_ceil(c, 32) // 32 * nks * 512))
        if case.down:
            krow = T.proj_krow(co)
            out["w_proj"] = (I.wp, dict(co=co, ci_total=ci, ks=1, mode=1, nseg=1, seg_off=0, seg_c=[ci], rows_pad=_ceil(ci, 16), k_pad=krow, numel=_ceil(ci, 16) * krow))
    return out


def build_images(lib, case, I):
    """One cgen_weight_prep launch for every image of the case; role -> device address.  Returns (addresses, what must stay alive)."""
    from causal_gen_amd import _lib

    descs = image_descs(case, I)
    total = sum(_ceil(f["numel"], 128) + SLACK for _, f in descs.values())
    buf = torch.full((total,), float("nan"), dtype=I.tdt, device="cuda")
    assert buf.data_ptr() % 256 == 0
    keep, table, csite, cidx, addr, off = [buf], [], [], [], {}, 0
    for i, (role, (src, f)) in enumerate(descs.items()):
        s = src.contiguous().cuda()
        keep.append(s)
        d = _lib.WprepDesc()
        d.src, d.dst = s.data_ptr(), buf.data_ptr() + 2 * off
        d.co, d.ci_total, d.ks, d.mode, d.nseg, d.seg_off = f["co"], f["ci_total"], f["ks"], f["mode"], f["nseg"], f["seg_off"]
        for k, c in enumerate(f["seg_c"]):
            d.seg_c[k] = c
        d.dtype, d.rows_pad, d.k_pad, d.numel = _lib.F16, f["rows_pad"], f["k_pad"], f["numel"]
        table.append(d)
        nch = -(-f["numel"] // 1024)
        csite += [i] * nch
        cidx += list(range(nch))
        addr[role] = d.dst
        off += _ceil(f["numel"], 128) + SLACK
    arr = (_lib.WprepDesc * len(table))(*table)
    tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    cs, cx = torch.tensor(csite, dtype=torch.int32, device="cuda"), torch.tensor(cidx, dtype=torch.int32, device="cuda")
    lib.weight_prep(tab.data_ptr(), cs.data_ptr(), cx.data_ptr(), len(csite), None)
    torch.cuda.synchronize()
    return addr, keep + [tab, cs, cx]


class Run:
    """The parents, views and argument record of one case."""

    def __init__(self, lib, case, I, images):
        self.lib, self.case, self.I = lib, case, I
        A = self.A = Arena(lib, case, None)
        assert A.tdt == I.tdt
        n, h, w = case.n, case.h, case.w
        ptr = dict(images)
        self.keep, self.views = [], {}

        def put(role, shape, values, out=False, planes=1):
            if shape[3] % 8:  # the parents: [n][8], zero padded, spatially constant
                vs = A.place((shape[0], 1, 1, 8), 0, (shape[0], 1, 1, shape[3]), values, zero_to=8)
            else:
                pshape, off = T.parent_shape(case, shape)
                vs = A.place(pshape, off, shape, values, out=out, planes=planes)
                m, v = T.view_of(case, vs[0].data_ptr(), shape), cv(vs[0])
                assert (m.sn, m.sh, m.sw, m.c) == (v.sn, v.sh, v.sw, v.c) and vs[0].data_ptr() % 16 == 0
            self.keep.append(vs)
            self.views[role] = vs
            ptr[role] = vs[0].data_ptr()
            return vs

        def vec(role, values):
            if values is None:
                return
            t = torch.full((values.numel() + 320,), float("nan"), device="cuda")
            t[:values.numel()] = values.cuda()
            assert t.data_ptr() % 16 == 0
            self.keep.append(t)
            ptr[role] = t.data_ptr()

        put("mid", (n, h, w, case.b), None, out=True)
        if case.dir == "fwd":
            for k, c in enumerate(case.segs):
                put(f"s{k}", (n, h, w, c), [I.segs[k]])
            vec("bias_a", I.bias_a)
            vec("bias0", I.bias_o)
            vec("bias_proj", I.bias_p)
            ho, wo = case.out_hw
            planes = 2 if case.rem else 1
            vs = put("out0", (n, ho, wo, case.co), None, out=True, planes=planes)
            if case.rem:
                ptr["rem_out"] = vs[1].data_ptr() - vs[0].data_ptr()
            if case.res1 == "own":
                vs = put("res0", (n, h, w, case.co), [I.res1, I.res1_rem][:planes], planes=planes)
                if case.rem:
                    ptr["rem_res"] = vs[1].data_ptr() - vs[0].data_ptr()
        else:
            put("s0", (n, h, w, case.co), [I.g])
            put("mid_aux", (n, h, w, case.b), [I.t])
            for j, k in enumerate(case.dsegs):
                shape = (n, h, w, case.segs[k])
                put(f"out{j}", shape, None, out=True)
                put(f"aux{j}", shape, [I.x[j]])
                if case.res1:
                    put(f"res{j}", shape, [I.res[j]])
        self.args = T.args(case, ptr)

    def call(self):
        self.lib.block3(ctypes.byref(self.args), None)
        torch.cuda.synchronize()

    def outputs(self):
        """[mid, out0 (, its remainder plane) (, out1)] as stored."""
        names = ["mid"] + [f"out{j}" for j in range(self.case.nout)]
        return [v for r in names for v in self.views[r]]


_REFS = {}


def _inputs(case, bf16):
    if case.id() not in _REFS:
        _REFS.clear()  # (one case at a time)
        I = R.make_inputs(case, bf16)
        _REFS[case.id()] = (I, R.stage1(case, I))
    return _REFS[case.id()]


def _held(name, got, ref, tdt, half_ulp_of=None):
    assert bool(torch.isfinite(got).all()), f"{name}: {int((~torch.isfinite(got)).sum())} elements are not finite: something from outside a view came in"
    w, bad = R.worst(got, ref, tdt, half_ulp_of)
    assert bad == 0, f"{name}: {bad} of {got.numel()} elements outside the bound (k {ref.k:g}), worst err/tol {w:.3f}"
    return w


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id())
def test_block3_against_f64(lib, case):
    I, ref1 = _inputs(case, lib.h16_is_bf16)  # (on the CPU, before anything runs on the GPU)
    tdt = I.tdt
    images, keep = build_images(lib, case, I)
    run = Run(lib, case, I, images)
    ok, key, vals = T.plan(lib, run.args)
    assert ok and key == case.key, f"cgen_block3_plan: {key}, the table expects {case.key}"
    assert {k: vals[k] for k in case.about} == case.about
    run.call()
    mid = run.views["mid"][0].cpu().double()
    w1 = _held("mid", mid, ref1, tdt)
    refs = R.stage2(case, I, mid)
    w2 = 0.0
    for j, ref in enumerate(refs):
        got = run.views[f"out{j}"][0].cpu().double()
        w2 = max(w2, _held(f"out{j}", got, ref, tdt))
        if case.rem:
            rem = run.views[f"out{j}"][1].cpu().double()
            assert bool(torch.isfinite(rem).all())
            assert bool(R.nearest16(got, rem, tdt).all()), "out is not the 16-bit value nearest to out + out_rem"
            w2 = max(w2, _held(f"out{j} + rem", got + rem, ref, tdt, half_ulp_of=rem))
    print(f"block3_f64 {case.family()} {case.id()} worst err/tol: mid {w1:.3f}, out {w2:.3f}")
    run.A.check_untouched()
    again = Run(lib, case, I, images)
    again.call()
    for a, b in zip(run.outputs(), again.outputs()):
        assert torch.equal(_bits(a), _bits(b)), "a second launch into fresh parents gives other bits"


# ------------------------------------------------------------------------------------------------- what a caller can be declined for
def _by_name(cid):
    return next(c for c in T.CASES if c.id() == cid)


def _declined():
    def misaligned(run, a):
        a.seg[0].p += 2

    def ragged_out(run, a):
        a.o[0].out.c = 12

    def second_bias(run, a):
        a.o[1].bias = a.w_a

    def down_fields(run, a):
        a.w_proj, a.proj_krow, a.pool = a.w_a, 64, 2

    tile = T.Case("t", "fwd", 2, 20, 28, [32], 8, 32)
    return [
        ("h-below-4", T.Case("h3", "fwd", 2, 3, 28, [32], 8, 32), None),
        ("misaligned-view", tile, misaligned),
        ("out-c-not-a-multiple-of-8", tile, ragged_out),
        ("second-output-with-a-bias", T.Case("n2", "dgrad", 2, 20, 28, [32, 32], 16, 32), second_bias),
        ("co-above-224-on-the-tile-kernel", T.Case("co232", "fwd", 2, 20, 28, [32], 8, 232), None),
        ("down-fields-on-a-tile-shape", tile, down_fields),
        ("down-fields-on-a-small-shape", T.Case("s", "fwd", 2, 12, 12, [32], 8, 32), down_fields),
    ]


@pytest.mark.parametrize("name,case,change", _declined(), ids=[d[0] for d in _declined()])
def test_declined_records_launch_nothing(lib, name, case, change):
    from causal_gen_amd import _lib

    I = R.make_inputs(case, lib.h16_is_bf16)
    images, keep = build_images(lib, case, I)
    run = Run(lib, case, I, images)
    if change is not None:
        change(run, run.args)
    out = (ctypes.c_int32 * T.PLAN_INTS)()
    assert lib.block3_supported(ctypes.byref(run.args)) == 0 and lib.block3_plan(ctypes.byref(run.args), out) == 0
    with pytest.raises(_lib.CgenError):
        lib.block3(ctypes.byref(run.args), None)
    torch.cuda.synchronize()
    for parent, v, before in run.A.outs:
        assert torch.equal(_bits(parent), _bits(before)), "a declined call wrote"
