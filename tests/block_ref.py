"""f64 references of the fused light Block (cgen_block3), forward and data gradient, for the cases of tests/block_cases.py: the inputs
of a case (drawn on the CPU from the case's id), the two-stage reference, the per-element bound, and the mutants the bound has to tell
from the reference.  Built on tests/conv_ref.py (input magnitudes, effective weights, the sequential f32 chain).

Two stages, because the bottleneck `mid` is WRITTEN (the weight gradients and the backward mask read it), so that no element of the
output bound has to absorb a 16-bit rounding flip in `mid`:
  stage 1   mid as stored, against
              forward  bias_a + conv3x3(relu(cat(seg)), w1_q)
              dgrad    conv3x3(g, w2 dgrad) * relu'(mid_aux),   relu'(x) = [x > 0]
  stage 2   o[k].out against the reference computed FROM THE mid THE KERNEL WROTE (read back):
              forward  bias + conv3x3(relu(mid), w2_q) + res1 (+ res1_rem)
              dgrad    conv3x3(mid, w1 dgrad of segment k) * relu'(aux_k) + res1_k
            Zero padding applies to mid itself: a bottleneck pixel outside the image is 0, not bias_a.
  down Block (csrc/block.hip header):
              forward  avg2x2( rn16( conv + bias + rn16(w_proj . seg[0] + bias_proj) ) )
              dgrad    rn16( conv * relu' + res1 ) + w_proj^T . g
w_q: the OIHW f32 parameter rounded to the 16-bit format (cgen_weight_prep rounds it into the image).

Bound per element:  |got - ref| <= T + 1/2 ulp16(|ref| + T),   T = k 2^-24 A + extra,   k = k_acc + k_epi
  A       the same formula on absolute values (relu' masks as they are);
  k_acc   K_ACC per kernel family: four times (conv_ref.K_MARGIN) the worst error of ONE k-ordered f32 fmaf chain (conv_ref.chain_error)
          over this table's own inputs, never more than the a-priori 2 L (L = 9 x the conv's input channels); the down Block's 1x1
          sum adds min(that, 2 c);
  k_epi   one per epilogue operation present: bias, mask product, res1, res1_rem; the down Block: + the projection's bias and its add,
          + 4 for the 2x2 average (three adds and the scaling);
  1/2 ulp the kernels round ONCE, to nearest (f2h_pk): half an output ulp, so that "rounds toward zero" is a detectable mutant;
  extra   internal roundings that are not stored, one full 16-bit ulp of the f64 value each, through the linear operation that follows:
          down forward avg2x2(ulp16(proj) + ulp16(conv + bias + proj)), down dgrad ulp16(conv * relu' + res1).  Nothing else.
Remainder planes: hi + rem is held to ref within T + 1/2 ulp16(rem), and hi is the 16-bit value nearest to hi + rem (`nearest16`: where
hi + rem lies exactly half way -- a remainder that itself rounded up to half an ulp -- either neighbour is nearest).

Not a mutant: a forward relu that lets a negative subnormal through as its value.  It moves an output by 2^-24 |w|, one f32 rounding of
a single product, below every term of the bound; relu' (the data gradient) passing it as 1 moves an output by the whole conv value."""
import math
import zlib
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from conv_cases import NONE, RELU
from conv_ref import K_MARGIN, U32, _conv, _mag, _nchw, _nhwc, chain_error, effective_weight, smallest_positive
from gpu_views import _ulp

# family -> 4 x the worst chain error measured by `python tests/block_ref.py` over both stages of every case of the table (the measured
# worst in the comment, in units of 2^-24 A; IEEE binary16 build)
K_ACC = {
    "tile": 19.0,   # measured 4.598
    "small": 16.0,  # measured 3.968
    "rows": 19.0,   # measured 4.550
}
CHAIN_BUDGET = 1 << 20


def tdt_of(bf16):
    return torch.bfloat16 if bf16 else torch.float16


def rn16(x, tdt):
    return x.to(torch.float32).to(tdt).double()


def rtz16(x, tdt):
    r = x.to(torch.float32).to(tdt)
    over = r.double().abs() > x.abs()
    return torch.where(over, torch.nextafter(r, torch.zeros_like(r)), r).double()


def ulp16(x, tdt):
    return _ulp(x.abs(), tdt)


def nearest16(hi, rem, tdt):
    """hi is a 16-bit value nearest to hi + rem."""
    v = hi + rem
    r = rn16(v, tdt)
    return (r == hi) | ((v - hi).abs() == (v - r).abs())


# ------------------------------------------------------------------------------------------------- inputs
def _plant(t, tdt):
    """0, -0 and the two smallest subnormals at a tile corner, in the last pixel and in the last channel."""
    n, h, w, c = t.shape
    s = smallest_positive(tdt)
    vals = [0.0, -0.0, s, -s]
    for i, v in enumerate(vals):
        t[0, min(7, h - 1), min(15, w - 1), (5 * i) % c] = v      # the last pixel of the first 8 x 16 tile ...
        t[0, min(8, h - 1), min(16, w - 1), c - 1 - i % c] = v    # ... the first of its diagonal neighbour, last channels
        t[n - 1, h - 1, w - 1, (c - 1 - i) % c] = v               # the last pixel
        t[n - 1, h // 2, max(w - 2 - i, 0), c - 1] = v            # the last channel


def make_inputs(case, bf16=False):
    """The operands of a case, NHWC f64 holding the stored values exactly (the parents: [n, 1, 1, c])."""
    tdt = tdt_of(bf16)
    g = torch.Generator().manual_seed(zlib.crc32(case.id().encode()))
    n, h, w, b, co = case.n, case.h, case.w, case.b, case.co
    ci = sum(case.segs)
    I = SimpleNamespace(tdt=tdt)
    I.w1 = (torch.randn((b, ci, 3, 3), generator=g, dtype=torch.float64) / math.sqrt(9 * ci)).float()
    I.w2 = (torch.randn((co, b, 3, 3), generator=g, dtype=torch.float64) / math.sqrt(9 * b)).float()
    I.w1q, I.w2q = I.w1.to(tdt).double(), I.w2.to(tdt).double()
    I.wp = I.wpq = I.bias_p = None
    if case.down:
        I.wp = (torch.randn((co, ci, 1, 1), generator=g, dtype=torch.float64) / math.sqrt(ci)).float()
        I.wpq = I.wp.to(tdt).double()
    if case.dir == "fwd":
        I.segs = []
        for c in case.segs:
            x = _mag(g, (n, 1, 1, c) if c % 8 else (n, h, w, c), tdt)
            if c % 8:
                x[n - 1, 0, 0, c - 1] = -0.0
            else:
                _plant(x, tdt)
            I.segs.append(x)
        I.bias_a = (torch.randn((b,), generator=g, dtype=torch.float64) * 0.5).float() if case.bias in ("both", "a") else None
        I.bias_o = (torch.randn((co,), generator=g, dtype=torch.float64) * 0.5).float() if case.bias in ("both", "o") else None
        if case.down and case.bias in ("both", "o"):
            I.bias_p = (torch.randn((co,), generator=g, dtype=torch.float64) * 0.5).float()
        I.res1 = I.res1_rem = None
        if case.res1 == "alias":
            I.res1 = I.segs[0]
        elif case.res1 == "own":
            if case.rem:  # a trunk value that needs more than the format's bits: hi + rem
                v = _mag(g, (n, h, w, co), torch.float32, 3.0)
                I.res1 = v.to(tdt).double()
                I.res1_rem = (v - I.res1).to(tdt).double()
            else:
                I.res1 = _mag(g, (n, h, w, co), tdt)
    else:
        I.g = _mag(g, (n, h, w, co), tdt)
        I.t = _mag(g, (n, h, w, b), tdt)
        _plant(I.t, tdt)
        I.x, I.res = [], []
        for k in case.dsegs:
            x = _mag(g, (n, h, w, case.segs[k]), tdt)
            _plant(x, tdt)
            I.x.append(x)
            I.res.append(_mag(g, (n, h, w, case.segs[k]), tdt) if case.res1 else None)
    return I


def images(case, I, sl):
    """The case and its inputs restricted to the images `sl` (a slice of the batch)."""
    J = SimpleNamespace(**vars(I))
    cut = lambda t: None if t is None else t[sl]
    if case.dir == "fwd":
        J.segs = [cut(x) for x in I.segs]
        J.res1, J.res1_rem = cut(I.res1), cut(I.res1_rem)
    else:
        J.g, J.t = cut(I.g), cut(I.t)
        J.x, J.res = [cut(x) for x in I.x], [cut(r) for r in I.res]
    return J


def _cat(case, I):
    n = I.segs[0].shape[0]
    return torch.cat([x.expand(n, case.h, case.w, x.shape[3]) for x in I.segs], dim=-1)


# ------------------------------------------------------------------------------------------------- the reference
def _pad_wrap(a):
    """Zero rows above and below; the column left of a row holds the previous row's last pixel, the one right of it the next row's
    first: what a kernel reads that takes x = -1 / x = W from the flattened image instead of zero."""
    n, c, h, w = a.shape
    flat = F.pad(a.reshape(n, c, h * w), (1, 1))
    left = flat[:, :, 0:h * w:w].unsqueeze(3)          # flat index y * w - 1 + 1
    right = flat[:, :, w + 1:h * w + 2:w].unsqueeze(3)  # flat index (y + 1) * w + 1
    return F.pad(torch.cat([left, a, right], dim=3), (0, 0, 1, 1))


def _tap_parity(a, wt):
    """The contribution of tap (0, 0) at the output pixels of parity (row, column) = (1, 0)."""
    n, c, h, w = a.shape
    sh = F.pad(a, (1, 1, 1, 1))[:, :, :h, :w]  # a[y - 1, x - 1]
    d = F.conv2d(sh, wt[:, :, :1, :1])
    m = torch.zeros((1, 1, h, w), dtype=d.dtype)
    m[:, :, 1::2, 0::2] = 1
    return d * m


def _conv_stage(a, a_abs, wt, mutant, tag):
    """conv3x3 of stage `tag` ("a" / "b") on operand a [n, C, h, w] with weight wt [oc, C, 3, 3]: (sum, sum of absolute values), the
    conv-level mutants applied where they name this stage; None where a mutant does not apply."""
    acc = _conv(a, wt, 3)
    A = _conv(a_abs, wt.abs(), 3)
    if mutant == tag + "_tap":
        acc = acc - _tap_parity(a, wt)
    elif mutant == "wrap_input" and tag == "a":
        acc = F.conv2d(_pad_wrap(a), wt)
    elif mutant == "kdrop" and tag == "a":
        if a.shape[1] <= 32:
            return None, None
        acc = acc - _conv(a[:, :32], wt[:, :32], 3)
    return acc, A


STAGE1_MUTANTS = ("a_tap", "wrap_input", "kdrop", "bias_a_last", "relu_neg_as_one", "relu_zero_as_one", "rtz")
STAGE2_MUTANTS = ("b_tap", "halo_bias", "res1_last_row", "swap_pair", "stale_mid", "relu_neg_as_one", "relu_zero_as_one", "rtz")


def _mask(x, mutant):
    m = x > 0
    if mutant == "relu_neg_as_one":
        m = m | (torch.signbit(x) & (x.abs() <= 2.0 ** -14))  # -0 and the negative subnormals pass
    elif mutant == "relu_zero_as_one":
        m = x >= 0
    return m.double()


def _k_acc(case, L):
    return min(K_ACC[case.family()], 2.0 * L)


def _finish(R, v, A, k, extra=None):
    R.ref, R.A, R.k = _nhwc(v), _nhwc(A), k
    R.extra = _nhwc(extra) if extra is not None else torch.zeros_like(R.ref)
    return R


def tolerance(R, tdt, half_ulp_of=None):
    T = R.k * U32 * R.A + R.extra
    at = R.ref.abs() + T if half_ulp_of is None else half_ulp_of.abs()
    return T + 0.5 * ulp16(at, tdt)


def worst(got, R, tdt, half_ulp_of=None):
    """(worst err / tol, elements outside) of got (f64) against the bound of R."""
    tol = tolerance(R, tdt, half_ulp_of)
    err = (got - R.ref).abs()
    bad = ~(err <= tol)
    return float((err / tol.clamp_min(1e-300)).max()), int(bad.sum())


def stage1(case, I, mutant=None):
    """The bottleneck as stored: SimpleNamespace(ref, A, extra, k), NHWC f64; None where `mutant` does not apply."""
    R = SimpleNamespace()
    if case.dir == "fwd":
        x = _nchw(_cat(case, I))
        a = torch.relu(x)
        acc, A = _conv_stage(a, a, I.w1q, mutant, "a")
        if acc is None:
            return None
        k_epi = 0
        if I.bias_a is not None:
            ba = I.bias_a.double().clone()
            if mutant == "bias_a_last":
                ba[-1] = 0
            acc, A, k_epi = acc + ba.view(1, -1, 1, 1), A + I.bias_a.double().abs().view(1, -1, 1, 1), 1
        elif mutant == "bias_a_last":
            return None
        if mutant in ("relu_neg_as_one", "relu_zero_as_one"):
            return None  # (forward: the module docstring)
        return _finish(R, acc, A, _k_acc(case, 9 * x.shape[1]) + k_epi)
    shim = SimpleNamespace(dir="dgrad", seg_off=0, out_c=case.b)
    wt = effective_weight(shim, SimpleNamespace(wq=I.w2q))  # [b, co, 3, 3]
    g = _nchw(I.g)
    acc, A = _conv_stage(g, g.abs(), wt, mutant, "a")
    if acc is None or mutant == "bias_a_last":
        return None
    t = _nchw(I.t)
    return _finish(R, acc * _mask(t, mutant), A * _mask(t, None), _k_acc(case, 9 * case.co) + 1)


def _stale(case, mid):
    """`mid` [n, h, w, b] with the bottleneck tile (halo included) of the FIRST tile of the second round of a persistent workgroup
    replaced by that of the tile the workgroup walked before it; None where no workgroup walks two tiles."""
    if case.family() != "tile" or case.about["ntiles"] <= case.about["grid"]:
        return None
    th, grid = case.key[5], case.about["grid"]
    tx_n, ty_n = -(-case.w // 16), -(-case.h // th)

    def where(t):
        return t // (tx_n * ty_n), (t // tx_n) % ty_n * th, t % tx_n * 16

    (n1, y1, x1), (n0, y0, x0) = where(grid), where(0)
    pad = F.pad(mid, (0, 0, 1, 17, 1, th + 1))  # zeros outside the image; the bottleneck tile of (y, x): rows y - 1 .. y + th, columns x - 1 .. x + 16
    out = pad.clone()
    out[n1, y1:y1 + th + 2, x1:x1 + 18] = pad[n0, y0:y0 + th + 2, x0:x0 + 18]
    return out[:, 1:1 + case.h, 1:1 + case.w], n1


def _swap_last_pair(v):
    """Two channels of the last (partial) 32-channel pair swapped."""
    c = v.shape[1]
    i, j = c - 1, max(c - 2, (c - 1) // 32 * 32)
    if i == j:
        return None
    v = v.clone()
    v[:, [i, j]] = v[:, [j, i]]
    return v


def stage2(case, I, mid, mutant=None):
    """One reference per output from `mid` (NHWC f64: what the kernel stored); None where `mutant` does not apply.  A reference of the
    mutant "stale_mid" covers one image only (.image)."""
    tdt = I.tdt
    image = None
    if mutant == "rtz" and case.down:
        return None  # (the down Block's two internal roundings are allowed a full ulp each: more than rounding toward zero costs)
    if mutant == "stale_mid":
        st = _stale(case, mid)
        if st is None:
            return None
        mid, image = st[0][st[1]:st[1] + 1], st[1]
        I = images(case, I, slice(image, image + 1))
    m = _nchw(mid)
    out = []
    if case.dir == "fwd":
        a = torch.relu(m)
        acc, A = _conv_stage(a, a, I.w2q, mutant, "b")
        if mutant == "halo_bias":
            if I.bias_a is None:
                return None
            n, c, h, w = a.shape
            frame = torch.relu(I.bias_a.double()).view(1, -1, 1, 1).expand(n, c, h + 2, w + 2).clone()
            frame[:, :, 1:-1, 1:-1] = a
            acc = F.conv2d(frame, I.w2q)
        k = _k_acc(case, 9 * case.b)
        if I.bias_o is not None:
            acc, A, k = acc + I.bias_o.double().view(1, -1, 1, 1), A + I.bias_o.double().abs().view(1, -1, 1, 1), k + 1
        extra = None
        if case.down:
            x = _nchw(_cat(case, I))
            P, PA = F.conv2d(x, I.wpq), F.conv2d(x.abs(), I.wpq.abs())
            k += min(K_ACC[case.family()], 2.0 * x.shape[1]) + 1 + 4
            if I.bias_p is not None:
                P, PA, k = P + I.bias_p.double().view(1, -1, 1, 1), PA + I.bias_p.double().abs().view(1, -1, 1, 1), k + 1
            acc, A = acc + P, A + PA
            extra = F.avg_pool2d(ulp16(P, tdt) + ulp16(acc, tdt), 2)
            acc, A = F.avg_pool2d(acc, 2), F.avg_pool2d(A, 2)
        if I.res1 is not None:
            r = _nchw(I.res1).clone()
            A, k = A + r.abs(), k + 1
            if mutant == "res1_last_row":
                r[0, :, -1, :16] = 0
            acc = acc + r
            if I.res1_rem is not None:
                acc, A, k = acc + _nchw(I.res1_rem), A + _nchw(I.res1_rem).abs(), k + 1
        elif mutant == "res1_last_row":
            return None
        if mutant in ("relu_neg_as_one", "relu_zero_as_one"):
            return None
        out.append(_finish(SimpleNamespace(), acc, A, k, extra))
    else:
        for j, kseg in enumerate(case.dsegs):
            shim = SimpleNamespace(dir="dgrad", seg_off=case.seg_off(kseg), out_c=case.segs[kseg])
            wt = effective_weight(shim, SimpleNamespace(wq=I.w1q))  # [c_k, b, 3, 3]
            acc, A = _conv_stage(m, m.abs(), wt, mutant, "b")
            if mutant == "halo_bias":
                return None
            x = _nchw(I.x[j])
            acc, A, k = acc * _mask(x, mutant), A * _mask(x, None), _k_acc(case, 9 * case.b) + 1
            if I.res[j] is not None:
                r = _nchw(I.res[j]).clone()
                A, k = A + r.abs(), k + 1
                if mutant == "res1_last_row":
                    r[0, :, -1, :16] = 0
                acc = acc + r
            elif mutant == "res1_last_row":
                return None
            extra = None
            if case.down:
                g = _nchw(I.g)
                wpt = I.wpq[:, :, 0, 0].t().contiguous().view(case.segs[kseg], case.co, 1, 1)
                extra = ulp16(acc, tdt)
                acc, A = acc + F.conv2d(g, wpt), A + F.conv2d(g.abs(), wpt.abs())
                k += min(K_ACC[case.family()], 2.0 * case.co) + 1
            out.append(_finish(SimpleNamespace(), acc, A, k, extra))
    if mutant == "swap_pair":
        for R in out:
            v = _swap_last_pair(_nchw(R.ref))
            if v is None:
                return None
            R.ref = _nhwc(v)
    for R in out:
        R.image = image
    return out


def stored(R, tdt, mutant=None):
    """What a kernel computing R.ref exactly would store."""
    return rtz16(R.ref, tdt) if mutant == "rtz" else rn16(R.ref, tdt)


# ------------------------------------------------------------------------------------------------- the sequential f32 chain
def chain_errors(case, I):
    """conv_ref.chain_error of the two convs of the case (the second on the 16-bit rounding of the first's reference)."""
    tdt = I.tdt
    sh = lambda **k: SimpleNamespace(ks=3, n=case.n, h=case.h, w=case.w, dt="h16", id=case.id, **k)
    mid = rn16(stage1(case, I).ref, tdt)
    errs = []
    if case.dir == "fwd":
        errs.append(chain_error(sh(dir="fwd", act=RELU), SimpleNamespace(segs=[_cat(case, I)], wq=I.w1q), CHAIN_BUDGET))
        errs.append(chain_error(sh(dir="fwd", act=RELU), SimpleNamespace(segs=[mid], wq=I.w2q), CHAIN_BUDGET))
    else:
        errs.append(chain_error(sh(dir="dgrad", act=NONE, seg_off=0, out_c=case.b), SimpleNamespace(segs=[I.g], wq=I.w2q), CHAIN_BUDGET))
        for k in case.dsegs:
            errs.append(chain_error(sh(dir="dgrad", act=NONE, seg_off=case.seg_off(k), out_c=case.segs[k]), SimpleNamespace(segs=[mid], wq=I.w1q), CHAIN_BUDGET))
    return max(errs)


def measure_k_acc(cases, bf16=False):
    out = {}
    for c in cases:
        e = chain_errors(c, make_inputs(c, bf16))
        out[c.family()] = max(out.get(c.family(), 0.0), e)
    return out


if __name__ == "__main__":
    from block_cases import CASES

    for fam, e in sorted(measure_k_acc(CASES).items()):
        print(f"{fam:6s} worst chain error {e:.3f} x 2^-24 A   -> k_acc >= {K_MARGIN * e:.2f}   (recorded {K_ACC[fam]})")
