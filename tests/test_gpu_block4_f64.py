"""cgen_block4 called through the C ABI -- the weight images from cgen_weight_prep modes 8-13, then ONE launch, no Engine -- on every
case of tests/block4_cases.py, against the staged f64 reference and the per-element bound of tests/block4_ref.py (its docstring derives
every term; tests/test_block4_cases.py keeps the CPU side: the mirror of the plan, instance keys, mutants, the measured constants).

Per case: cgen_block4_plan names the instance the table expects, before anything is launched; every element of mid[0], mid[1], mid[2]
and of every output meets the bound of its stage, each stage's reference computed from the tensor the kernel wrote for the stage
before; the flagged share of every forward operand, recomputed from the stored tensors, is within conv_ref.FLAG_SHARE_MAX; the padding
channels [b, ceil8(b)) of every mid are exactly zero; remainder planes hold hi + rem to the bound with hi a nearest 16-bit value;
nothing is NaN; nothing outside the output views changes; a second launch into fresh parents gives the same bits.

Layout: every view lies in a parent that is NaN wherever the view is not (tests/gpu_views.Arena.place) -- other images, rows, columns and
channels; only the channels [c, ceil8(c)) of a ragged INPUT view hold zeros, as cgen_view.cpad promises (an output's are NaN until the
kernel writes its zeros).  The kernel forms no address outside a view: out-of-image and padding loads come from 32 bytes of zeros
(g_b4zero), every store is predicated on the pixel and on the channel group lying below ceil8(c).  Weight images and biases get NaN
behind their last value, so that a fragment or a bias fetched from past the end would show the same way."""
import ctypes

import pytest
import torch

import block4_cases as T
import block4_ref as R
from block_cases import cp8, parent_shape
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
    nmb, g16 = _ceil(b, 32) // 32, _ceil(b, 16) // 16
    c3 = dict(co=b, ci_total=b, ks=3, nseg=1, seg_off=0, seg_c=[b], k_pad=g16, numel=nmb * 9 * g16 * 512)
    out = {}
    if case.dir == "fwd":
        nch = sum(_ceil(c, 32) // 32 for c in case.segs)
        out["w0"] = (I.W[0], dict(mode=8, co=b, ci_total=ci, ks=1, nseg=len(case.segs), seg_off=0, seg_c=case.segs, k_pad=2 * nch, numel=nmb * nch * 2 * 512))
        out["w1"] = (I.W[1], dict(c3, mode=10))
        out["w2"] = (I.W[2], dict(c3, mode=10))
        out["wo0"] = (I.W[3], dict(mode=12, co=co, ci_total=b, ks=1, nseg=1, seg_off=0, seg_c=[b], k_pad=g16, numel=_ceil(co, 32) // 32 * g16 * 512))
    else:
        nch = _ceil(co, 32) // 32
        out["w0"] = (I.W[3], dict(mode=9, co=co, ci_total=b, ks=1, nseg=1, seg_off=0, seg_c=[b], k_pad=2 * nch, numel=nmb * nch * 2 * 512))
        out["w1"] = (I.W[2], dict(c3, mode=11))
        out["w2"] = (I.W[1], dict(c3, mode=11))
        for j, k in enumerate(case.dsegs):
            c = case.segs[k]
            out[f"wo{j}"] = (I.W[0], dict(mode=13, co=b, ci_total=ci, ks=1, nseg=1, seg_off=case.seg_off(k), seg_c=[c], k_pad=g16, numel=_ceil(c, 32) // 32 * g16 * 512))
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
        d.dtype, d.rows_pad, d.k_pad, d.numel = _lib.F16, 0, f["k_pad"], f["numel"]
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
        n, h, w, b = case.n, case.h, case.w, case.b
        ptr = dict(images)
        self.keep, self.views, self.out_cpad = [], {}, []

        def put(role, shape, values, out=False, planes=1, seg=False):
            c = shape[3]
            if seg and case.flat(c):  # the parents: [n][8], zero padded, spatially constant
                vs = A.place((shape[0], 1, 1, cp8(c)), 0, (shape[0], 1, 1, c), values, zero_to=cp8(c))
            else:
                pshape, off = parent_shape(case, shape)
                vs = A.place(pshape, off, shape, values, out=out, planes=planes, zero_to=0 if out else cp8(c))
                m, v = T.view_of(case, vs[0].data_ptr(), shape), cv(vs[0])
                assert (m.sn, m.sh, m.sw, m.c) == (v.sn, v.sh, v.sw, v.c) and vs[0].data_ptr() % 16 == 0
                if out:
                    self.out_cpad += [cp8(c)] * planes
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

        for k in range(3):
            put(f"mid{k}", (n, h, w, b), None, out=True)
        if case.dir == "fwd":
            for k, c in enumerate(case.segs):
                put(f"s{k}", (n, h, w, c), [I.segs[k]], seg=True)
            for k in range(3):
                vec(f"bias{k}", I.bias[k])
            vec("biaso", I.bias[3])
            planes = 2 if "o" in case.rem else 1
            vs = put("out0", (n, h, w, case.co), None, out=True, planes=planes)
            if planes == 2:
                ptr["rem_out"] = vs[1].data_ptr() - vs[0].data_ptr()
            if case.res[0]:
                planes = 2 if "r" in case.rem else 1
                vs = put("res0", (n, h, w, case.co), [I.res1, I.res1_rem][:planes], planes=planes)
                if planes == 2:
                    ptr["rem_res"] = vs[1].data_ptr() - vs[0].data_ptr()
        else:
            put("s0", (n, h, w, case.co), [I.g])
            for k in range(3):
                put(f"aux{k}", (n, h, w, b), [I.aux[k]])
            for j, k in enumerate(case.dsegs):
                shape = (n, h, w, case.segs[k])
                put(f"out{j}", shape, None, out=True)
                put(f"oaux{j}", shape, [I.x[j]])
                if case.res[j]:
                    put(f"res{j}", shape, [I.res[j]])
        self.args = T.args(case, ptr)

    def call(self):
        self.lib.block4(ctypes.byref(self.args), None)
        torch.cuda.synchronize()

    def outputs(self):
        """[mid0, mid1, mid2, out0 (, its remainder plane) (, out1 ..)] as stored."""
        names = ["mid0", "mid1", "mid2"] + [f"out{j}" for j in range(self.case.nout)]
        return [v for r in names for v in self.views[r]]

    def parents(self):
        return [p for p, _, _ in self.A.outs]


_INPUTS = {}


def _inputs(case, bf16):
    if case.id() not in _INPUTS:
        _INPUTS.clear()  # (one case at a time)
        _INPUTS[case.id()] = R.make_inputs(case, bf16)
    return _INPUTS[case.id()]


def _held(name, got, ref, tdt, half_ulp_of=None):
    assert bool(torch.isfinite(got).all()), f"{name}: {int((~torch.isfinite(got)).sum())} elements are not finite: something from outside a view came in"
    w, bad = R.worst(got, ref, tdt, half_ulp_of)
    assert bad == 0, f"{name}: {bad} of {got.numel()} elements outside the bound (k {ref.k:g}), worst err/tol {w:.3f}"
    return w


def _pad_is_zero(run, k):
    """The channels [b, ceil8(b)) of mid[k], which lie behind the view in its parent."""
    case = run.case
    if case.b % 8 == 0:
        return
    v = run.views[f"mid{k}"][0]
    pad = torch.as_strided(v, (case.n, case.h, case.w, cp8(case.b) - case.b), v.stride(), v.storage_offset() + case.b)
    assert bool((pad == 0).all()), f"mid[{k}]: the padding channels are not zero"


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id())
def test_block4_against_f64(lib, case):
    I = _inputs(case, lib.h16_is_bf16)  # (on the CPU, before anything runs on the GPU)
    tdt = I.tdt
    images, keep = build_images(lib, case, I)
    run = Run(lib, case, I, images)
    ok, key, vals = T.plan(lib, run.args)
    assert ok == 1 and key == case.key, f"cgen_block4_plan: {key}, the table expects {case.key}"
    assert (key, vals) == T.mirror(run.args)
    run.call()
    worst, prev = [], None
    for s in range(3):
        ref = R.stage(case, I, s, prev)
        assert ref.flag_share <= R.FLAG_SHARE_MAX, f"stage {s}: {ref.flag_share:.4f} of the operand the kernel stored is flagged"
        got = run.views[f"mid{s}"][0].cpu().double()
        worst.append(_held(f"mid[{s}]", got, ref, tdt))
        _pad_is_zero(run, s)
        prev = got
    w3 = 0.0
    for j in range(case.nout):
        ref = R.stage(case, I, 3, prev, j=j)
        assert ref.flag_share <= R.FLAG_SHARE_MAX
        got = run.views[f"out{j}"][0].cpu().double()
        w3 = max(w3, _held(f"out{j}", got, ref, tdt))
        if "o" in case.rem:
            rem = run.views[f"out{j}"][1].cpu().double()
            assert bool(torch.isfinite(rem).all())
            assert bool(R.nearest16(got, rem, tdt).all()), "out is not a 16-bit value nearest to out + out_rem"
            w3 = max(w3, _held(f"out{j} + rem", got + rem, ref, tdt, half_ulp_of=rem))
    print(f"block4_f64 {case.id()} {key} worst err/tol: mid {worst[0]:.3f} {worst[1]:.3f} {worst[2]:.3f}, out {w3:.3f}")
    run.A.check_untouched(cpad=run.out_cpad)
    again = Run(lib, case, I, images)
    again.call()
    for a, b in zip(run.parents(), again.parents()):
        nan = torch.isnan(a)
        assert torch.equal(nan, torch.isnan(b)) and torch.equal(_bits(a)[~nan], _bits(b)[~nan]), "a second launch into fresh parents gives other bits"


@pytest.mark.parametrize("pair", T.PAIRS, ids=lambda p: f"nb8-{p[0].key[1]}")
def test_block4_pair_is_byte_equal_to_two_single_launches(lib, pair):
    ins = [R.make_inputs(c, lib.h16_is_bf16) for c in pair]
    imgs = [build_images(lib, c, I) for c, I in zip(pair, ins)]
    single = [Run(lib, c, I, im[0]) for c, I, im in zip(pair, ins, imgs)]
    paired = [Run(lib, c, I, im[0]) for c, I, im in zip(pair, ins, imgs)]
    out = (ctypes.c_int32 * T.PLAN_INTS)()
    a, b = paired[0].args, paired[1].args
    assert lib.block4_pair_supported(ctypes.byref(a), ctypes.byref(b)) == 1 and lib.block4_pair_plan(ctypes.byref(a), ctypes.byref(b), out) == 1
    assert tuple(out[1:5]) == (pair[0].key[1], 4, pair[0].ntiles, pair[0].ntiles + pair[1].ntiles)
    for r in single:
        r.call()
    lib.block4_pair(ctypes.byref(a), ctypes.byref(b), None)
    torch.cuda.synchronize()
    for r, q in zip(single, paired):
        for x, y in zip(r.outputs(), q.outputs()):
            assert bool(torch.isfinite(x).all()) and torch.equal(_bits(x), _bits(y)), "the pair launch gives other bits than the single launch"
        q.A.check_untouched(cpad=q.out_cpad)


# ------------------------------------------------------------------------------------------------- what a caller is declined for
_DECL = [d for d in T.DECLINED if d[3]]


@pytest.mark.parametrize("name,base,change,gpu", _DECL, ids=[d[0] for d in _DECL])
def test_declined_records_launch_nothing(lib, name, base, change, gpu):
    from causal_gen_amd import _lib

    I = _inputs(base, lib.h16_is_bf16)
    images, keep = build_images(lib, base, I)
    run = Run(lib, base, I, images)
    change(run.args)
    out = (ctypes.c_int32 * T.PLAN_INTS)()
    assert lib.block4_supported(ctypes.byref(run.args)) == 0 and lib.block4_plan(ctypes.byref(run.args), out) == 0
    with pytest.raises(_lib.CgenError):
        lib.block4(ctypes.byref(run.args), None)
    torch.cuda.synchronize()
    for parent, v, before in run.A.outs:
        assert torch.equal(_bits(parent), _bits(before)), "a declined call wrote"
