"""f64 references of cgen_conv2d, forward and data gradient, for the cases of tests/conv_cases.py: the inputs of a case (drawn on the
CPU from the case's id, so that the GPU test and the CPU checks of tests/test_conv_cases.py see the same numbers), the reference and its
absolute companion, the tolerance, the mutants the tolerance has to tell from the reference, and the emulation of one sequential f32
accumulation chain from which the accumulation term of the tolerance is measured.

Everything is computed from the exact values of the operands AS STORED (f32, or the library's 16-bit format):

  forward   ref = conv2d(act(cat(x)), w_q, padding = ks // 2) + bias + res1 (+ res1_rem) + res2
  dgrad     ref = (conv_transpose2d(g, w_q[:, off:off + c_k], padding = ks // 2)) * act'(aux) + res1 (+ res1_rem)

w_q is the OIHW f32 weight rounded to the 16-bit format for "h16" (cgen_weight_prep rounds it into the image).  Both directions run as
one conv2d with an effective weight (the data gradient's is the flipped transpose: tests/test_conv_cases.py holds that to
conv_transpose2d and to autograd).  A is the same formula on absolute values -- gelu(|x|) for an activated operand and
Phi(|x|) + |x| phi(x), the derivative's terms without their cancellation, for act' (the form tests/test_gpu_elementwise.py uses: the f32
error of erff and expf is absolute in Phi, and gelu'(-3) = -0.012 is the difference of 0.0013 and 0.013).

Tolerance: |got - ref| <= k 2^-24 A + extra + one output ulp (tests/gpu_views.assert_bounded; `extra` is folded into A), with
k = k_acc + k_epi (+ k_split):
  k_acc    per arm family, K_ACC below: four times the worst error of ONE k-ordered f32 fmaf chain (`chain_error`) over the table's
           own inputs, in units of 2^-24 A, and never more than the a-priori 2 L (L = ks ks sum(c) products per output);
  k_epi    one per epilogue operation present (bias, the act' product, res1, res2, res1_rem), + 16 where an f32 erff GELU or GELU' is
           applied (the k tests/test_gpu_elementwise.py gives GELU);
  k_split  12 L for "f32s": two operands cut to 22 bits each and the low-by-low product dropped, at most 3 * 2^-22 per product.
16-bit GELU in the forward operand: the kernels' erf is Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7, so 7.5e-8 on Phi) or erff, and
16 f32 roundings are allowed on top: the kernel's activated value lies within delta = |x| (7.5e-8 + 16 * 2^-24) of the f64 one BEFORE it
is rounded to 16 bits.  Where no rounding midpoint lies within delta of the f64 value both round alike and the operand is exact;
elsewhere (the flagged elements) the two may differ by delta + one 16-bit ulp -- one ulp wherever delta is below half an ulp, several
subnormal ulps for gelu(-5) = -1.4e-6 -- and `extra` gets conv(flag * (ulp(a) + delta), |w|), nothing anywhere else.
16-bit GELU' in the data gradient: extra = |acc64| (1 + |aux|) (7.5e-8 + 16 * 2^-24)."""
import math
import zlib

import torch
import torch.nn.functional as F

from conv_cases import GELU, NONE, RELU, family

U32 = 2.0 ** -24
GELU16_DELTA = 7.5e-8 + 16 * U32
K_MARGIN = 4
# family -> 4 x the worst chain error measured by `python tests/conv_ref.py` over every case of the table (the measured worst in the
# comment, in units of 2^-24 A; IEEE binary16 build -- the bfloat16 build's inputs differ only in their rounding)
K_ACC = {
    "f32-gen": 15.0,   # measured 3.607
    "f32-tile": 17.0,  # measured 4.047
    "h16-gen": 18.0,   # measured 4.495
    "h16-tile": 17.0,  # measured 4.202
    "h16-px": 19.0,    # measured 4.697
    "h16-ws": 16.0,    # measured 3.938
    "h16-smlp": 20.0,  # measured 4.862
}


def tdt_of(dt, bf16):
    return torch.float32 if dt != "h16" else (torch.bfloat16 if bf16 else torch.float16)


def smallest_positive(tdt):
    return {torch.float32: 2.0 ** -149, torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133}[tdt]


def _gelu64(x):
    return 0.5 * x * (1 + torch.erf(x * math.sqrt(0.5)))


def _gelu_abs(x):
    return _gelu64(x.abs())


def _dgelu64(x):
    return 0.5 * (1 + torch.erf(x * math.sqrt(0.5))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def _dgelu_abs(x):
    return 0.5 * (1 + torch.erf(x * math.sqrt(0.5)).abs()) + x.abs() * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


class Inputs:
    pass


def _mag(g, shape, tdt, scale=1.0, p_neg=0.5):
    """Magnitudes uniform in [0.5, 1.5] with random signs, as stored in `tdt`, in f64."""
    v = (0.5 + torch.rand(shape, generator=g, dtype=torch.float64)) * scale
    v = torch.where(torch.rand(shape, generator=g, dtype=torch.float64) < p_neg, -v, v)
    return v.to(torch.float32).to(tdt).double()


def _plant(t, act, tdt):
    """Directed values from the middle of the tensor's flattened (n, h, w, c) order on, and in its last element."""
    flat = t.view(-1)
    mid = flat.numel() // 2
    if act == RELU:
        vals = [0.0, -0.0, smallest_positive(tdt), -smallest_positive(tdt)]
    elif act == GELU:
        vals = [0.0, -0.0, 8.0, -8.0, 5.0, -5.0, 3.0, -3.0, 0.75, -0.75]
    else:
        return
    for i, v in enumerate(vals):
        if mid + 2 * i + 1 < flat.numel() - 1:
            flat[mid + 2 * i + 1] = v
    if flat.numel() > 4:
        flat[-1] = vals[1 + (flat.numel() % 3)]


FLAG_SHARE_MAX = 0.01


def make_inputs(case, bf16=False):
    """The operands of a case, NHWC, in f64 holding the stored values exactly.  A 16-bit GELU operand is drawn from the first seed
    (the case's id, then id + 1 ...) that keeps the flagged elements of the module docstring within FLAG_SHARE_MAX."""
    for salt in range(64):
        I = _make_inputs(case, bf16, salt)
        if not (case.dir == "fwd" and case.act == GELU and case.dt == "h16") or activated(case, I)[3] <= FLAG_SHARE_MAX:
            break
    return I


def _make_inputs(case, bf16, salt):
    tdt = tdt_of(case.dt, bf16)
    g = torch.Generator().manual_seed(zlib.crc32(case.id().encode()) + salt)
    I = Inputs()
    I.tdt, I.salt = tdt, salt
    n, h, w = case.n, case.h, case.w
    # A 16-bit GELU operand is negative with probability 1 / 4 only: gelu(x) on [-1.5, -0.5] is -0.10 .. -0.17, eight times smaller than
    # |x| and with a 16-bit ulp as much finer, so that in binary16 2.3 % of the negative operands lie within delta of a midpoint against
    # 0.4 % of the positive ones; evenly split signs flag 1.3 % of a large tensor whatever the seed, three to one 0.9 %
    p_neg = 0.25 if (case.dir == "fwd" and case.act == GELU and case.dt == "h16") else 0.5
    I.segs = [_mag(g, (n, h, w, c), tdt, p_neg=p_neg) for c in case.in_segs]
    if case.dir == "fwd":
        _plant(I.segs[0], case.act, tdt)
    ci = sum(case.segs)
    L = case.ks * case.ks * (ci if case.dir == "fwd" else case.co)
    I.w = (torch.randn((case.co, ci, case.ks, case.ks), generator=g, dtype=torch.float64) / math.sqrt(L)).float()  # the OIHW parameter
    I.wq = I.w.to(tdt).double()
    oc = case.out_c
    I.bias = (torch.randn((oc,), generator=g, dtype=torch.float64) * 0.5).float() if case.bias else None
    I.aux = I.res1 = I.res2 = I.res1_rem = None
    if case.has_aux:
        I.aux = _mag(g, (n, h, w, oc), tdt)
        _plant(I.aux, case.act, tdt)
    if case.res1:
        if case.res1_rem:  # a trunk value that needs more than the format's bits: hi + rem
            v = _mag(g, (n, h, w, oc), torch.float32, 3.0)
            I.res1 = v.to(tdt).double()
            I.res1_rem = (v - I.res1).to(tdt).double()
        else:
            I.res1 = _mag(g, (n, h, w, oc), tdt)
    if case.res2:
        I.res2 = _mag(g, (n, h, w, oc), tdt)
    return I


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def effective_weight(case, I, flip=True):
    """[out_c, in_c, ks, ks] of the conv2d both directions run as."""
    if case.dir == "fwd":
        return I.wq
    wk = I.wq[:, case.seg_off:case.seg_off + case.out_c]  # [co, c_k, ks, ks]
    if flip:
        wk = wk.flip(2, 3)
    return wk.transpose(0, 1).contiguous()


def _neighbours(r16):
    up = torch.nextafter(r16, torch.full_like(r16, float("inf")))
    dn = torch.nextafter(r16, torch.full_like(r16, float("-inf")))
    return up.double(), dn.double()


def activated(case, I):
    """The conv's operand in NCHW: (a, |.| companion, per-element 16-bit shift allowance or None, flagged share)."""
    x = _nchw(torch.cat(I.segs, dim=-1))
    act = case.act if case.dir == "fwd" else NONE
    if act == NONE:
        return x, x.abs(), None, 0.0
    if act == RELU:
        a = torch.relu(x)
        return a, a, None, 0.0
    g64 = _gelu64(x)
    if case.dt != "h16":
        return g64, _gelu_abs(x), None, 0.0
    r16 = g64.to(I.tdt)
    r = r16.double()
    up, dn = _neighbours(r16)
    delta = x.abs() * GELU16_DELTA
    near = torch.minimum((g64 - (r + up) / 2).abs(), (g64 - (r + dn) / 2).abs()) <= delta
    near &= delta > 0
    ulp = torch.maximum(up - r, r - dn)
    return r, _gelu_abs(x), near * (ulp + delta), float(near.double().mean())


class Ref:
    pass


def _conv(a, w, ks):
    return F.conv2d(a, w, None, padding=ks // 2)


def reference(case, I, mutant=None):
    """Ref with .ref, .A, .extra (NHWC f64) and .k.  `mutant`: one of MUTANTS -- then .ref is the mutated reference, or None where
    the mutation does not apply to the case (it would leave the reference as it is)."""
    ks, p = case.ks, case.ks // 2
    a, a_abs, shift, share = activated(case, I)
    w = effective_weight(case, I, flip=mutant != "no_flip")
    R = Ref()
    R.flag_share = share
    n, C, H, W = a.shape
    centre_only = H == 1 and W == 1 and ks > 1  # (the kernels then run the centre tap alone)
    if mutant is None or mutant == "no_flip":
        if mutant == "no_flip" and (case.dir != "dgrad" or ks == 1):
            return None
        acc = _conv(a, w, ks)
    else:
        acc = R_acc = _conv(a, w, ks)
        if mutant == "drop_last_channel":
            ends = [sum(case.in_segs[:i + 1]) - 1 for i in range(len(case.in_segs))]
            acc = R_acc - _conv(a[:, ends], w[:, ends], ks)
        elif mutant == "drop_corner_tap":
            if ks == 1 or centre_only:
                return None
            sh = F.pad(a, (p, p, p, p))[:, :, :H, :W]  # a[y - p, x - p]: what tap (0, 0) multiplies
            acc = R_acc - F.conv2d(sh, w[:, :, :1, :1])
        elif mutant == "replicate_halo":
            if ks == 1:
                return None
            ap = F.pad(F.pad(a, (p, 0, 0, 0), mode="replicate"), (0, p, p, p))  # left side replicated, zeros elsewhere
            acc = R_acc.clone()
            acc[..., :p] = F.conv2d(ap[..., :3 * p], w)
        elif mutant == "drop_last_kstep":
            taps = [(ks // 2, ks // 2)] if centre_only else [(dy, dx) for dy in range(ks) for dx in range(ks)]
            order = [(dy, dx, c) for (dy, dx) in taps for c in range(C)][-32:]  # the kernels' K order: tap-major, channels inside
            m = torch.zeros_like(w)
            for dy, dx, c in order:
                m[:, c, dy, dx] = 1
            ch = sorted({c for _, _, c in order})
            acc = R_acc - _conv(a[:, ch], (w * m)[:, ch], ks)
        elif mutant in ("drop_bias_last_group", "drop_res2", "shift_dact"):
            pass
        else:
            raise KeyError(mutant)
    v = acc
    A = _conv(a_abs, w.abs(), ks)
    acc_abs = A
    k_epi = 0
    oc = case.out_c
    if I.bias is not None:
        b = I.bias.double().clone()
        if mutant == "drop_bias_last_group":
            b[(oc - 1) // 8 * 8:] = 0
        v = v + b.view(1, -1, 1, 1)
        A = A + I.bias.double().abs().view(1, -1, 1, 1)
        k_epi += 1
    elif mutant == "drop_bias_last_group":
        return None
    extra = torch.zeros_like(A)
    if shift is not None:
        extra = extra + _conv(shift, w.abs(), ks)
    if I.aux is not None:
        x = _nchw(I.aux)
        if case.act == RELU:
            d = (x > 0).double()
            dab = d
        else:
            d, dab = _dgelu64(x), _dgelu_abs(x)
            if case.dt == "h16":
                extra = extra + v.abs() * (1 + x.abs()) * GELU16_DELTA
            else:
                k_epi += 16
        if mutant == "shift_dact":
            d = torch.roll(d, 1, dims=-1)
        v, A = v * d, A * dab
        k_epi += 1
    elif mutant == "shift_dact":
        return None
    if case.dir == "fwd" and case.act == GELU and case.dt != "h16":
        k_epi += 16
    for t, name in ((I.res1, "res1"), (I.res1_rem, "res1_rem"), (I.res2, "res2")):
        if t is not None:
            if not (name == "res2" and mutant == "drop_res2"):
                v = v + _nchw(t)
            A = A + _nchw(t).abs()
            k_epi += 1
    if mutant == "drop_res2" and I.res2 is None:
        return None
    L = case.L()
    R.k_acc = min(K_ACC[family(case)], 2.0 * L)
    R.k_epi = k_epi
    R.k_split = 12.0 * L if case.dt == "f32s" else 0.0
    R.k = R.k_acc + R.k_epi + R.k_split
    R.ref, R.A, R.extra = _nhwc(v), _nhwc(A), _nhwc(extra)
    R.A_tol = R.A + R.extra / (R.k * U32)  # (assert_bounded takes k 2^-24 A: the absolute term rides in A)
    return R


MUTANTS = ("drop_last_channel", "drop_corner_tap", "replicate_halo", "drop_bias_last_group", "drop_last_kstep", "drop_res2", "no_flip",
           "shift_dact")


# ------------------------------------------------------------------------------------------------- the sequential f32 chain
def chain_error(case, I, budget=1 << 22, seed=0):
    """Worst |chain - exact| / (2^-24 A) of one k-ordered f32 fmaf chain (acc = float32(acc + a_k w_k), k = (tap, channel) as the weight
    image orders them) over the case's own operands rounded to f32, against the exact sum of the same products.  Every output of a case
    of up to `budget` multiply-adds; of a larger one, as many pixels (drawn from the case's id) as the budget allows, every channel."""
    ks, p = case.ks, case.ks // 2
    a, _, _, _ = activated(case, I)
    a = F.pad(a.float(), (p, p, p, p))
    w = effective_weight(case, I).float()  # [oc, C, ks, ks]
    n, C, H, W = case.n, a.shape[1], case.h, case.w
    P, oc, L = n * H * W, w.shape[0], C * ks * ks
    S = max(1, min(P, budget // (L * oc)))
    g = torch.Generator().manual_seed(zlib.crc32(case.id().encode()) + seed)
    pix = torch.randperm(P, generator=g)[:S] if S < P else torch.arange(P)
    nn, yy, xx = pix // (H * W), pix % (H * W) // W, pix % W
    cols = torch.stack([a[nn, :, yy + dy, xx + dx] for dy in range(ks) for dx in range(ks)], dim=1).reshape(S, L).double()  # tap-major
    wm = w.permute(2, 3, 1, 0).reshape(L, oc).double()
    acc = torch.zeros((S, oc), dtype=torch.float32)
    for k in range(L):
        acc = (acc.double() + cols[:, k:k + 1] * wm[k:k + 1]).float()  # (the product of two f32 is exact in f64)
    exact, A = cols @ wm, cols.abs() @ wm.abs()
    return float(((acc.double() - exact).abs() / (U32 * A).clamp_min(1e-300)).max())


def measure_k_acc(cases, bf16=False, budget=1 << 22):
    worst = {}
    for c in cases:
        e = chain_error(c, make_inputs(c, bf16), budget)
        f = family(c)
        worst[f] = max(worst.get(f, 0.0), e)
    return worst


if __name__ == "__main__":
    from conv_cases import CASES

    for fam, e in sorted(measure_k_acc(CASES).items()):
        print(f"{fam:10s} worst chain error {e:.3f} x 2^-24 A   -> k_acc >= {K_MARGIN * e:.2f}   (recorded {K_ACC[fam]})")
