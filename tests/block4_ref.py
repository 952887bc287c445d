"""f64 references of the fused default Block (cgen_block4), forward and data gradient, for the cases of tests/block4_cases.py: the
inputs of a case (drawn on the CPU from the case's id), the STAGED reference, the per-element bound, the f32 mirror of the kernel's
GELU table, and the mutants the bound has to tell from the reference.  Built on tests/conv_ref.py and tests/block_ref.py.

Four stages, because all three bottleneck tensors are WRITTEN and each phase reads the 16-bit value the one before it stored: stage s is
compared against f64 computed from the tensor the kernel wrote for stage s - 1 (read back), so that no element has to absorb a 16-bit
rounding flip of an earlier stage.  With a(v) = rn16(gelu(v)), zero outside the image, and Wq the OIHW f32 parameter rounded to 16 bits:
  forward   t0 = b0 + W0q . a(cat(x))      t1 = b1 + W1q * a(t0)      t2 = b2 + W2q * a(t1)      out = b3 + W3q . a(t2) + res1 (+ res1_rem)
  dgrad     g2 = (W3q^T . g) gelu'(t2)     g1 = (W2q^T * g2) gelu'(t1)   g0 = (W1q^T * g1) gelu'(t0)
            out_k = (W0q[:, k]^T . g0) gelu'(x_k) (+ res_k)      (* a 3x3 with zero padding, ^T * its flipped transpose; the operand
            between two stages is the stored rn16 value itself)

Bound per element:  |got - ref| <= T + 1/2 ulp16(|ref| + T),   T = k 2^-24 A + extra,   k = k_acc + k_epi       (as tests/block_ref.py)
  A       the same formula on absolute values: gelu(|v|) rounded for an activated operand, Phi(|x|) + |x| phi(x) for gelu';
  k_acc   K_ACC per phase kind -- "p0" the 1x1 from global memory, "c3" a 3x3 from LDS, "p3" the 1x1 to the outputs: K_MARGIN times the
          worst error of ONE k-ordered f32 fmaf chain (conv_ref.chain_error) over this table's own operands, never above 2 L;
  k_epi   one per epilogue operation present: a bias, the gelu' product, res1, res1_rem;
  1/2 ulp the kernel rounds ONCE, to nearest (f2h_pk).
GELU by table.  The kernel takes Phi(x) (forward) and gelu'(x) (data gradient) from a 385-entry second-order Taylor table (b4_lut_fill,
b4_lut).  `lut` is its f32 mirror; `measure_lut` runs it over every finite 16-bit input against f64:
  DELTA_FWD = K_MARGIN x the worst |Phi_table - Phi|, DELTA_BWD = K_MARGIN x the worst |gelu'_table - gelu'|, neither below the truncation
  figure the kernel's header states (2.5e-7, 8e-7).  The mirror builds the table with the host's erf and exp; the device's erff and
  __expf cannot be measured without a GPU, and the factor K_MARGIN stands for them.
  forward   the kernel's activated value, BEFORE it is rounded to 16 bits, lies within delta = |x| DELTA_FWD + 2^-24 |gelu(x)| (the f32
            product's rounding) of the f64 one.  Where no rounding midpoint lies within delta of the f64 value both round alike and the
            operand is exact; elsewhere (the flagged elements) the two may differ by one 16-bit ulp + delta, and `extra` gets
            conv(flag (ulp + delta), |w|) -- nothing anywhere else.  The flagged share of every stage's operand is at most
            conv_ref.FLAG_SHARE_MAX: a condition on the inputs (`make_inputs` takes the first seed that keeps it strictly), asserted again
            on the GPU from the stored tensors.
  dgrad     extra = |conv| DELTA_BWD, no flags.
Remainder planes: hi + rem is held to ref within T + 1/2 ulp16(rem), and hi is a 16-bit value nearest to hi + rem (block_ref.nearest16).

Inputs.  gelu(x) for x < 0 is small against |x|, so its 16-bit grid is fine against delta: a tensor with evenly split signs flags 2-3 %
of its elements in binary16.  The segments are therefore negative with probability 1 / 4 (conv_ref.make_inputs), and the weights carry a
positive mean (MU[k] / L per tap) beside their noise, so that t0 .. t2 are mostly positive and of order 1 to 2: the condition above is then met by the first
seed of almost every case."""
import math
import zlib
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from block_ref import nearest16, rn16, rtz16, tdt_of, tolerance, ulp16, worst, _tap_parity  # noqa: F401  (re-exported)
from conv_cases import NONE
from conv_ref import FLAG_SHARE_MAX, K_MARGIN, U32, _dgelu64, _dgelu_abs, _gelu64, _mag, _neighbours, _nchw, _nhwc, chain_error, effective_weight

# phase kind -> K_MARGIN x the worst chain error measured by `python tests/block4_ref.py` over every stage of every case of the table
# (the measured worst in the comment, in units of 2^-24 A; IEEE binary16 build)
K_ACC = {
    "p0": 30.0,  # measured 7.420
    "c3": 28.0,  # measured 6.903
    "p3": 24.0,  # measured 5.958
}
# K_MARGIN x the worst error of the table mirror over all finite 16-bit inputs (`python tests/block4_ref.py`; measured in the comment,
# binary16 / bfloat16 inputs), not below the kernel header's truncation figures
DELTA_FWD = 1.2e-6   # measured 2.993e-7 / 2.783e-7
DELTA_BWD = 4.3e-6   # measured 1.074e-6 / 1.037e-6
TRUNC_FWD, TRUNC_BWD = 2.5e-7, 8e-7
CHAIN_BUDGET = 1 << 20
MU = (3.0, 1.0, 1.0, 1.0)      # mean of a forward weight, times the conv's L: t = MU mean(a) + noise stays near 1.6 at every stage,
SIGMA = (0.5, 0.3, 0.3, 0.3)   # where Phi and its table still move (gelu is the identity from 4 on); noise of a forward weight, times sqrt(L)
KIND = ("p0", "c3", "c3", "p3")


# ------------------------------------------------------------------------------------------------- the table mirror
def _f32(x):
    return x.to(torch.float32)


def lut_tables(fwd):
    """b4_lut_fill in f32: [385, 3]."""
    i = torch.arange(385, dtype=torch.float32)
    x0 = (i - 192) * _f32(torch.tensor(1.0 / 32.0))
    cdf = 0.5 * (1 + torch.erf(x0 * _f32(torch.tensor(0.70710678118654752440))))
    pdf = _f32(torch.tensor(0.39894228040143267794)) * torch.exp(-0.5 * x0 * x0)
    if fwd:
        c = (cdf, pdf * (1.0 / 32.0), -x0 * pdf * (0.5 / 1024.0))
    else:
        c = (cdf + x0 * pdf, pdf * (2 - x0 * x0) * (1.0 / 32.0), pdf * (x0 * x0 * x0 - 4 * x0) * (0.5 / 1024.0))
    return torch.stack([_f32(v) for v in c], dim=1)


def lut(x, table, off=0):
    """b4_lut in f32 on x (any float dtype; returns f64 holding f32 values).  off: the mutant that reads the neighbouring entry."""
    t = _f32(x).clamp(-6, 6) * 32
    r = torch.round(t)  # (rint: to nearest even, like torch.round)
    d = (t - r).double()
    c = table[(r.long() + 192 + off).clamp(0, 384)].double()
    inner = _f32(d * c[..., 2] + c[..., 1]).double()  # (fmaf: one rounding)
    return _f32(d * inner + c[..., 0]).double()


_TAB = {}


def _table(fwd):
    if fwd not in _TAB:
        _TAB[fwd] = lut_tables(fwd)
    return _TAB[fwd]


def _phi64(x):
    return 0.5 * (1 + torch.erf(x * math.sqrt(0.5)))


def all_finite16(tdt):
    v = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(tdt)
    return v[torch.isfinite(v)].double()


def measure_lut(tdt):
    """(worst |Phi_table - Phi|, worst |gelu'_table - gelu'|) over every finite value of the 16-bit format."""
    x = all_finite16(tdt)
    return (float((lut(x, _table(True)) - _phi64(x)).abs().max()), float((lut(x, _table(False)) - _dgelu64(x)).abs().max()))


# ------------------------------------------------------------------------------------------------- operands
def activate(x, tdt, mutant=None):
    """The forward MFMA operand of the stored tensor x (f64): (a = rn16(gelu(x)), |.| companion, flagged shift allowance, flagged share)."""
    g64 = _gelu64(x)
    r16 = _f32(g64).to(tdt)
    r = r16.double()
    if mutant == "lut_off":
        return rn16(_f32(x.double() * lut(x, _table(True), off=1)).double(), tdt), None, None, 0.0
    up, dn = _neighbours(r16)
    delta = x.abs() * DELTA_FWD + g64.abs() * U32
    near = torch.minimum((g64 - (r + up) / 2).abs(), (g64 - (r + dn) / 2).abs()) <= delta
    near &= delta > 0
    ulp = torch.maximum(up - r, r - dn)
    return r, rn16(_gelu64(x.abs()), tdt), near * (ulp + delta), float(near.double().mean())


def dgelu(x, mutant=None):
    if mutant == "dgelu_phi":
        return _phi64(x)
    if mutant == "lut_off":
        return lut(x, _table(False), off=1)
    return _dgelu64(x)


# ------------------------------------------------------------------------------------------------- inputs
GELU_VALUES = [0.0, -0.0, 8.0, -8.0, 5.0, -5.0, 3.0, -3.0, 0.75, -0.75]


def _plant(t):
    """Directed GELU arguments from the middle of the tensor on, and in its last pixel -- in tensors of at least 2048 elements: most of
    the negative ones are flagged (gelu(-5) = -1.4e-6 has subnormal ulps below delta), and ten of them in a 24-element tensor are no
    share a seed can bring under the cap."""
    flat = t.view(-1)
    if flat.numel() < 2048:
        return
    mid = flat.numel() // 2
    for i, v in enumerate(GELU_VALUES):
        if mid + 2 * i + 1 < flat.numel() - 1:
            flat[mid + 2 * i + 1] = v
    if flat.numel() > 4:
        flat[-1] = GELU_VALUES[1 + flat.numel() % 3]


def _weight(g, shape, L, tdt, fwd, k):
    w = torch.randn(shape, generator=g, dtype=torch.float64) * (SIGMA[k] if fwd else 1.0) / math.sqrt(L) + (MU[k] / L if fwd else 0.0)
    w = w.float()
    return w, w.to(tdt).double()


def _draw(case, bf16, salt):
    tdt = tdt_of(bf16)
    g = torch.Generator().manual_seed(zlib.crc32(case.id().encode()) + salt)
    n, h, w, b, co = case.n, case.h, case.w, case.b, case.co
    ci = sum(case.segs)
    fwd = case.dir == "fwd"
    I = SimpleNamespace(tdt=tdt, salt=salt)
    I.W, I.Wq = [None] * 4, [None] * 4
    for k, (shape, L) in enumerate((((b, ci, 1, 1), ci), ((b, b, 3, 3), 9 * b), ((b, b, 3, 3), 9 * b), ((co, b, 1, 1), b))):
        I.W[k], I.Wq[k] = _weight(g, shape, L, tdt, fwd, k)
    if fwd:
        I.segs = []
        for c in case.segs:
            x = _mag(g, (n, 1, 1, c) if case.flat(c) else (n, h, w, c), tdt, p_neg=0.25)
            if not case.flat(c):
                _plant(x)
            I.segs.append(x)
        I.bias = [(torch.randn((b if k < 3 else co,), generator=g, dtype=torch.float64) * 0.5).float() if case.bias[k] == "1" else None for k in range(4)]
        I.res1 = I.res1_rem = None
        if case.res[0]:
            if "r" in case.rem:  # a trunk value that needs more than the format's bits: hi + rem
                v = _mag(g, (n, h, w, co), torch.float32, 3.0)
                I.res1 = v.to(tdt).double()
                I.res1_rem = (v - I.res1).to(tdt).double()
            else:
                I.res1 = _mag(g, (n, h, w, co), tdt)
    else:
        I.g = _mag(g, (n, h, w, co), tdt)
        I.aux = []  # mid_aux[0 .. 2] = the forward t2, t1, t0
        for k in range(3):
            t = _mag(g, (n, h, w, b), tdt)
            _plant(t)
            I.aux.append(t)
        I.x, I.res = [], []
        for j, k in enumerate(case.dsegs):
            x = _mag(g, (n, h, w, case.segs[k]), tdt)
            _plant(x)
            I.x.append(x)
            I.res.append(_mag(g, (n, h, w, case.segs[k]), tdt) if case.res[j] else None)
    return I


def make_inputs(case, bf16=False):
    """The operands of a case, NHWC f64 holding the stored values exactly.  Forward: the first seed (the case's id, then id + 1 ...) for
    which the reference's own operands -- the drawn segments and the reference's rounded t0 .. t2 -- keep every stage's flagged share
    strictly below FLAG_SHARE_MAX."""
    for salt in range(64):
        I = _draw(case, bf16, salt)
        if case.dir != "fwd":
            return I
        prev, shares, room = None, [], []
        for s in range(4):
            R = stage(case, I, s, prev)
            shares.append(R.flag_share)
            # (t0 .. t2 as the kernel stores them may differ from the reference's in an element here and there: one element to spare --
            #  where one element is less than half the cap; in a smaller tensor the cap already means that nothing is flagged)
            room.append(R.flag_share + (1.0 / prev.numel() if s and prev.numel() > 2 / FLAG_SHARE_MAX else 0.0))
            prev = rn16(R.ref, I.tdt)
        if max(room) < FLAG_SHARE_MAX:
            I.flag_shares = shares
            return I
    raise AssertionError(f"{case.id()}: no seed keeps the flagged share below {FLAG_SHARE_MAX}")


def images(case, I, sl):
    """The inputs restricted to the images `sl` (a slice of the batch)."""
    J = SimpleNamespace(**vars(I))
    cut = lambda t: None if t is None else t[sl]
    if case.dir == "fwd":
        J.segs = [cut(x) for x in I.segs]
        J.res1, J.res1_rem = cut(I.res1), cut(I.res1_rem)
    else:
        J.g, J.aux = cut(I.g), [cut(t) for t in I.aux]
        J.x, J.res = [cut(x) for x in I.x], [cut(r) for r in I.res]
    return J


def _cat(case, segs):
    n = segs[0].shape[0]
    return torch.cat([x.expand(n, case.h, case.w, x.shape[3]) for x in segs], dim=-1)


# ------------------------------------------------------------------------------------------------- the reference
# mutant -> the stages it changes (forward, data gradient); a stage function answers None where the mutant leaves the case as it is
MUTANTS = {
    "tap": ((1, 2), (1, 2)),             # one tap of a 3x3 dropped at one parity
    "halo_gelu_bias": ((1, 2), ()),      # an out-of-image bottleneck pixel holds gelu(bias), not 0 (after phase 0: stage 1; after phase 1: stage 2)
    "bias_last": ((0, 1, 2), ()),        # the last bottleneck channel's bias missing
    "chunk_hi": ((0,), (0,)),            # channels 16 .. 31 of a segment's last 32-channel chunk dropped
    "chunk_first": ((0,), (0,)),         # the last segment's first chunk dropped
    "seg_alias": ((0,), ()),             # segment 1 read through segment 0's pixel pointer
    "dgelu_phi": ((), (0, 1, 2, 3)),     # gelu' reduced to Phi
    "dgelu_neighbour": ((), (0, 1, 2)),  # gelu' taken from the neighbouring stage's aux
    "lut_off": ((0, 1, 2, 3), (0, 1, 2, 3)),  # the table read one entry off
    "res1_last_row": ((3,), (3,)),       # res1 dropped in the last row of the first tile
    "res1_rem": ((3,), ()),              # the remainder plane of res1 dropped
    "acc_out1": ((), (3,)),              # the accumulate dropped on output 1 of several
    "swap_pair": ((0, 1, 2, 3), (0, 1, 2, 3)),  # two channels of the last (partial) 32-row block swapped
    "rtz": ((0, 1, 2, 3), (0, 1, 2, 3)),  # the output rounded toward zero
}


def _conv(a, w):
    return F.conv2d(a, w, None, padding=w.shape[2] // 2)


def _swap_last_pair(v):
    c = v.shape[1]
    if c < 2:
        return None
    v = v.clone()
    v[:, [c - 1, c - 2]] = v[:, [c - 2, c - 1]]
    return v


def _drop_channels(case, s, mutant):
    """Input channels of stage 0 that the chunk mutants drop (indices on the concatenated axis), or None."""
    widths = case.segs if case.dir == "fwd" else [case.co]
    offs = [sum(widths[:k]) for k in range(len(widths))]
    if mutant == "chunk_first":
        return list(range(offs[-1], offs[-1] + min(32, widths[-1])))
    for off, c in zip(offs, widths):
        lo = (c - 1) // 32 * 32 + 16
        if c > lo:
            return list(range(off + lo, off + c))
    return None


def _finish(v, A, k, extra, share=0.0):
    return SimpleNamespace(ref=_nhwc(v), A=_nhwc(A), k=k, extra=_nhwc(extra), flag_share=share)


def _k_acc(s, L):
    return min(K_ACC[KIND[s]], 2.0 * L)


def stage_operand(case, I, s, prev):
    """The tensor stage s reads, NHWC f64 as stored: the inputs for stage 0, else `prev` (what stage s - 1 stored)."""
    if s > 0:
        return prev
    return _cat(case, I.segs) if case.dir == "fwd" else I.g


def stage_weight(case, I, s, j=0):
    """[out, in, ks, ks] of the conv2d stage s runs as (output j of stage 3)."""
    if case.dir == "fwd":
        return I.Wq[s]
    if s < 3:
        src = I.Wq[3 - s]
        return effective_weight(SimpleNamespace(dir="dgrad", seg_off=0, out_c=src.shape[1]), SimpleNamespace(wq=src))
    k = case.dsegs[j]
    return effective_weight(SimpleNamespace(dir="dgrad", seg_off=case.seg_off(k), out_c=case.segs[k]), SimpleNamespace(wq=I.Wq[0]))


def stage(case, I, s, prev=None, mutant=None, j=0):
    """The reference of stage s (0 .. 2: mid[s]; 3: output j) computed from `prev`, the tensor stage s - 1 stored (NHWC f64):
    SimpleNamespace(ref, A, extra, k, flag_share).  With a mutant: the mutated reference, or None where it does not apply."""
    fwd = case.dir == "fwd"
    tdt = I.tdt
    if mutant is not None and s not in MUTANTS[mutant][0 if fwd else 1]:
        return None
    x = _nchw(stage_operand(case, I, s, prev))
    w = stage_weight(case, I, s, j)
    if mutant == "seg_alias":
        if len(case.segs) < 2:
            return None
        c0, c1 = case.segs[0], case.segs[1]
        x = x.clone()
        x[:, c0:c0 + c1] = 0
        x[:, c0:c0 + min(c0, c1)] = _nchw(_cat(case, I.segs[:1]))[:, :min(c0, c1)]
    L = w.shape[1] * w.shape[2] * w.shape[3]
    if fwd:
        a, a_abs, shift, share = activate(x, tdt, mutant)
        if shift is None:
            a_abs, shift = a.abs(), torch.zeros_like(a)
    else:
        a, a_abs, shift, share = x, x.abs(), None, 0.0
    acc, A = _conv(a, w), _conv(a_abs, w.abs())
    extra = _conv(shift, w.abs()) if shift is not None else torch.zeros_like(A)
    if mutant == "tap":
        if a.shape[2] < 2 or a.shape[3] < 3:
            return None  # (tap (0, 0) of the pixels (odd row, even column) reads inside the image from 2 x 3 pixels on)
        acc = acc - _tap_parity(a, w)
    elif mutant in ("chunk_hi", "chunk_first"):
        ch = _drop_channels(case, s, mutant)
        if ch is None:
            return None
        acc = acc - _conv(a[:, ch], w[:, ch])
    elif mutant == "halo_gelu_bias":
        bprev = I.bias[s - 1]
        if bprev is None:
            return None
        n, c, h, wd = a.shape
        frame = activate(bprev.double(), tdt)[0].view(1, -1, 1, 1).expand(n, c, h + 2, wd + 2).clone()
        frame[:, :, 1:-1, 1:-1] = a
        acc = F.conv2d(frame, w)
    k = _k_acc(s, L)
    if fwd:
        bias = I.bias[s]
        if bias is not None:
            bq = bias.double().clone()
            if mutant == "bias_last":
                bq[-1] = 0
            acc, A, k = acc + bq.view(1, -1, 1, 1), A + bias.double().abs().view(1, -1, 1, 1), k + 1
        elif mutant == "bias_last":
            return None
        res, rem = (I.res1, I.res1_rem) if s == 3 else (None, None)
    else:
        aux = I.aux[s] if s < 3 else I.x[j]
        if mutant == "dgelu_neighbour":
            aux = I.aux[(s + 1) % 3]
        d = dgelu(_nchw(aux), mutant)
        extra = extra + acc.abs() * DELTA_BWD
        acc, A, k = acc * d, A * _dgelu_abs(_nchw(aux)), k + 1
        res, rem = (I.res[j], None) if s == 3 else (None, None)
    if res is not None:
        r = _nchw(res).clone()
        A, k = A + r.abs(), k + 1
        if mutant == "res1_last_row":
            r[0, :, min(7, r.shape[2] - 1), :16] = 0
        if mutant == "acc_out1":
            if j != 1:
                return None
            r = r * 0
        acc = acc + r
        if rem is not None:
            A, k = A + _nchw(rem).abs(), k + 1
            if mutant != "res1_rem":
                acc = acc + _nchw(rem)
        elif mutant == "res1_rem":
            return None
    elif mutant in ("res1_last_row", "res1_rem", "acc_out1"):
        return None
    if mutant == "swap_pair":
        acc = _swap_last_pair(acc)
        if acc is None:
            return None
    return _finish(acc, A, k, extra, share)


def stored(R, tdt, mutant=None):
    """What a kernel computing R.ref exactly would store."""
    return rtz16(R.ref, tdt) if mutant == "rtz" else rn16(R.ref, tdt)


def reference_chain(case, I):
    """[R0, R1, R2, [R3 per output]] with every stage computed from the 16-bit rounding of the reference before it."""
    out, prev = [], None
    for s in range(3):
        R = stage(case, I, s, prev)
        out.append(R)
        prev = rn16(R.ref, I.tdt)
    out.append([stage(case, I, 3, prev, j=j) for j in range(case.nout)])
    return out


# ------------------------------------------------------------------------------------------------- the sequential f32 chain
def chain_errors(case, I, budget=CHAIN_BUDGET):
    """phase kind -> conv_ref.chain_error of the stages of that kind, on the operands the reference chain feeds them."""
    tdt = I.tdt
    errs, prev = {}, None
    for s in range(4):
        x = _nchw(stage_operand(case, I, s, prev))
        a = activate(x, tdt)[0] if case.dir == "fwd" else x
        for j in range(case.nout if s == 3 else 1):
            w = stage_weight(case, I, s, j)
            shim = SimpleNamespace(ks=w.shape[2], n=case.n, h=case.h, w=case.w, dt="h16", id=case.id, dir="fwd", act=NONE)
            e = chain_error(shim, SimpleNamespace(segs=[_nhwc(a)], wq=w, tdt=tdt), budget)
            errs[KIND[s]] = max(errs.get(KIND[s], 0.0), e)
        if s < 3:
            prev = rn16(stage(case, I, s, prev).ref, tdt)
    return errs


def measure_k_acc(cases, bf16=False, budget=CHAIN_BUDGET):
    out = {}
    for c in cases:
        for kind, e in chain_errors(c, make_inputs(c, bf16), budget).items():
            out[kind] = max(out.get(kind, 0.0), e)
    return out


if __name__ == "__main__":
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # (the package, as tests/conftest.py finds it)
    from block4_cases import CASES

    for kind, e in sorted(measure_k_acc(CASES).items()):
        print(f"{kind:3s} worst chain error {e:.3f} x 2^-24 A   -> k_acc >= {K_MARGIN * e:.2f}   (recorded {K_ACC[kind]})")
    for name, tdt in (("binary16", torch.float16), ("bfloat16", torch.bfloat16)):
        f, b = measure_lut(tdt)
        print(f"{name}: table mirror worst |Phi error| {f:.3e} -> delta_fwd >= {max(K_MARGIN * f, TRUNC_FWD):.3e} (recorded {DELTA_FWD});"
              f"  worst |gelu' error| {b:.3e} -> delta_bwd >= {max(K_MARGIN * b, TRUNC_BWD):.3e} (recorded {DELTA_BWD})")
    shares = [max(make_inputs(c).flag_shares) for c in CASES if c.dir == "fwd"]
    print(f"flagged share, worst stage of every forward case: max {max(shares):.4f} (cap {FLAG_SHARE_MAX})")
