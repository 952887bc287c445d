"""f64 reference of cgen_conv2d_wgrad + cgen_wgrad_reduce for the cases of tests/wgrad_cases.py: the inputs of a case (drawn on the CPU
from the case's id, so that tests/test_gpu_wgrad_f64.py and the CPU checks of tests/test_wgrad_cases.py see the same numbers), the
reference with its absolute companion, the tolerance, the mutants the tolerance has to tell from the reference, and the sequential f32
chain from which the accumulation term of the tolerance is measured.

Everything is computed from the exact values of the operands AS STORED (f32, or the library's 16-bit format):

  grad_w[co][ci][dy][dx] = prev + unscale * sum_px g[px][co] * a[px + (dy, dx) - ks // 2][ci]      a = act(cat(x)), zeros outside the image
  grad_b[co]             = prev + unscale * sum_px g[px][co]

that is d/dW and d/db of sum(g * conv2d(a, W, b, padding = ks // 2)) (tests/test_wgrad_cases.py holds it to autograd).  `prev` only where
the reduce accumulates; unscale is a power of two, applied exactly.  A is the same formula on absolute values, gelu(|x|) for an activated
operand, |prev| included.

The activated operand follows the kernel that serves the case (cgen_conv2d_wgrad_plan_record, tests/wgrad_cases.plan):
  kind 0  wgrad_kernel applies act_fwd in f32 and feeds the f32 MFMA: the operand is NOT rounded to 16 bits.  GELU is erff's: the kernel's
          value lies within 16 * 2^-24 * gelu(|x|) of the f64 one (the bound tests/test_gpu_elementwise.py holds cgen_unary_fwd to), and
          `extra` = sum_px |g| * that.
  kind 1  wgrad_tile_kernel activates the staged tile in place, in the 16-bit format: the operand is rounded.  ReLU is exact.  GELU as in
          tests/conv_ref.py: the kernel's value lies within delta = |x| GELU16_DELTA of the f64 one before the rounding; where no
          rounding midpoint lies within delta both round alike, elsewhere (the flagged elements, at most FLAG_SHARE_MAX of a tensor)
          `extra` gets |g| (ulp + delta).

Tolerance per element: |got - ref| <= K_ACC[family] 2^-24 A + extra + (P + 2) 2^-149.  The last term is the f32 format's floor: the ReLU
cases plant the smallest positive value of the format, and a column whose other operands ReLU zeroes has A = |g| 2^-149 -- no f32 result
can lie within 2^-24 of that; each of the P products and the two roundings of the reduce may be off by one subnormal step (or flushed).
K_ACC is measured, not chosen: K_MARGIN (4) times the worst
|chain - exact| / (2^-24 A) of ONE sequential f32 fmaf chain over the pixel axis (`chain_error`) over every case of the table, rounded
up.  The margin covers what the chain does not model: the MFMA's internal order, the K-way combine through LDS, the splits and the
four-chain reduce, the product with unscale and the sum with prev."""
import math
import zlib

import torch
import torch.nn.functional as F

import wgrad_cases as T
from conv_ref import FLAG_SHARE_MAX, GELU16_DELTA, K_MARGIN, _gelu64, _gelu_abs, _mag, _neighbours, _plant, tdt_of
from wgrad_cases import GELU, NONE, RELU

U32 = 2.0 ** -24
# family -> K_MARGIN x the worst chain error measured by `python tests/wgrad_ref.py` over every case of the table, rounded up (the
# measured worst in the comment, in units of 2^-24 A; IEEE binary16 build)
K_ACC = {
    "f32-gen": 11.0,   # measured 2.671
    "h16-gen": 17.0,   # measured 4.173
    "h16-tile": 17.0,  # measured 4.109
}


class Inputs:
    pass


def _kind(case):
    return T.plan(T.problem(case))["kind"]


def make_inputs(case, bf16=False):
    """The operands of a case, NHWC, in f64 holding the stored values exactly.  A 16-bit GELU operand of the tiled kernel is drawn from
    the first seed (the case's id, then id + 1 ...) that keeps the flagged elements within FLAG_SHARE_MAX."""
    rounded_gelu = case.act == GELU and _kind(case) == 1
    for salt in range(64):
        I = _make_inputs(case, bf16, salt, 0.25 if rounded_gelu else 0.5)  # (conv_ref.make_inputs on why one in four is negative)
        if not rounded_gelu or activated(case, I, 1)[3] <= FLAG_SHARE_MAX:
            break
    return I


def _make_inputs(case, bf16, salt, p_neg):
    tdt = tdt_of(case.dt, bf16)
    g = torch.Generator().manual_seed(zlib.crc32(case.id().encode()) + salt)
    I = Inputs()
    I.tdt, I.salt = tdt, salt
    n, h, w = case.n, case.h, case.w
    I.segs = []
    for s, c in enumerate(case.segs):
        if case.v(s).bcast:  # spatially constant (the parents)
            I.segs.append(_mag(g, (n, 1, 1, c), tdt, p_neg=p_neg).expand(n, h, w, c).contiguous())
        else:
            I.segs.append(_mag(g, (n, h, w, c), tdt, p_neg=p_neg))
    _plant(I.segs[0], case.act, tdt)
    I.g = _mag(g, (n, h, w, case.co), tdt, 0.5)
    ci = sum(case.segs)
    I.prev_w = I.prev_b = None
    if case.accumulate:  # of the size of a typical sum of unscale * P products
        sc = case.unscale * math.sqrt(n * h * w) * 0.5
        I.prev_w = (torch.randn((case.co, ci, case.ks, case.ks), generator=g, dtype=torch.float64) * sc).float().double()
        I.prev_b = (torch.randn((case.co,), generator=g, dtype=torch.float64) * sc).float().double()
    return I


def activated(case, I, kind, skip=None, flip_rounding=False):
    """The operand in NHWC: (a, |.| companion, per-element allowance or None, flagged share).  `skip`: a segment left as it is.
    `flip_rounding`: rounded to 16 bits where the kernel does not round, and the other way about."""
    outs = [[], [], []]
    share_n = share_d = 0
    rounded = (kind == 1) != flip_rounding
    for s, x in enumerate(I.segs):
        act = NONE if s == skip else case.act
        allow = torch.zeros_like(x)
        if act == NONE:
            a, ab = x, x.abs()
        elif act == RELU:
            a = torch.relu(x)
            ab = a
        else:
            a, ab = _gelu64(x), _gelu_abs(x)
            if kind == 0:
                allow = 16 * U32 * ab
            else:
                r16 = a.to(I.tdt)
                r = r16.double()
                up, dn = _neighbours(r16)
                delta = x.abs() * GELU16_DELTA
                near = (torch.minimum((a - (r + up) / 2).abs(), (a - (r + dn) / 2).abs()) <= delta) & (delta > 0)
                allow = near * (torch.maximum(up - r, r - dn) + delta)
                share_n, share_d = share_n + int(near.sum()), share_d + near.numel()
        if rounded and act != NONE:
            a = a.to(I.tdt).double() if I.tdt != torch.float32 else a.to(torch.float16).double()
        outs[0].append(a), outs[1].append(ab), outs[2].append(allow)
    a, ab, allow = (torch.cat(o, dim=-1) for o in outs)
    return a, ab, (allow if bool((allow != 0).any()) else None), (share_n / share_d if share_d else 0.0)


def wgrad(g, a, ks, replicate_left=False):
    """[co][ci][ks][ks] = sum_px g[px][co] a[px + tap - ks // 2][ci], from NHWC f64."""
    n, h, w, co = g.shape
    p = ks // 2
    an = a.permute(0, 3, 1, 2)
    if replicate_left and p:
        ap = F.pad(F.pad(an, (p, 0, 0, 0), mode="replicate"), (0, p, p, p))
    else:
        ap = F.pad(an, (p, p, p, p))
    ap = ap.permute(0, 2, 3, 1)
    G = g.reshape(-1, co).t().contiguous()
    out = torch.empty((co, a.shape[3], ks, ks), dtype=torch.float64)
    for dy in range(ks):
        for dx in range(ks):
            out[:, :, dy, dx] = G @ ap[:, dy:dy + h, dx:dx + w, :].reshape(n * h * w, -1)
    return out


def split_of_pixels(case, plan):
    """[n, h, w] -> the split that accumulates the pixel, and (kind 0) its 64-pixel K-step inside the split / (kind 1) its tile."""
    n, h, w = case.n, case.h, case.w
    px = torch.arange(n * h * w).view(n, h, w)
    if plan["kind"] == 0:
        sp = px // plan["pix_per_split"]
        return sp, (px - sp * plan["pix_per_split"]) // T.WG_PK
    tx, ty = T._ceil_div(w, T.TILE_W), T._ceil_div(h, T.TILE_H)
    nn, yy, xx = px // (h * w), px % (h * w) // w, px % w
    tile = (nn * ty + yy // T.TILE_H) * tx + xx // T.TILE_W
    return tile // plan["tps"], tile


MUTANTS = ("drop_last_pixel", "drop_last_kstep_of_last_split", "drop_corner_tap", "drop_last_tap_group", "replicate_halo",
           "drop_last_channel_of_segment", "shift_segment_offset", "act_skips_a_segment", "act_rounded_to_16_bits", "act_not_rounded",
           "drop_last_split", "bias_misses_last_image", "no_accumulate")
# the kinds a mutant is meaningful for
MUTANT_KINDS = {m: (0, 1) for m in MUTANTS}
MUTANT_KINDS.update(drop_last_tap_group=(0,), act_rounded_to_16_bits=(0,), act_not_rounded=(1,))


class Ref:
    pass


def reference(case, I, plan=None, mutant=None):
    """Ref with .w, .b (None without a bias), .A_w, .A_b, .tol_w, .tol_b, .k, .flag_share.  `mutant`: one of MUTANTS -- then the mutated
    reference, or None where the mutation does not apply to the case (it would leave the reference as it is)."""
    plan = plan or T.plan(T.problem(case))
    kind, ks = plan["kind"], case.ks
    assert kind in (0, 1)
    if mutant is not None and kind not in MUTANT_KINDS[mutant]:
        return None
    n, h, w = case.n, case.h, case.w
    skip = None
    if mutant == "act_skips_a_segment":
        if case.act == NONE:
            return None
        skip = len(case.segs) - 1
    flip = mutant in ("act_rounded_to_16_bits", "act_not_rounded")
    if flip and (case.act == NONE or (case.act == RELU and case.dt == "h16")):
        return None  # (nothing to round: ReLU of a 16-bit value is a 16-bit value)
    a, a_abs, allow, share = activated(case, I, kind, skip, flip)
    g, gb = I.g, I.g
    sp, sub = split_of_pixels(case, plan)
    last = sp == plan["nsplit"] - 1
    if mutant == "drop_last_pixel":
        g = g.clone()
        g[-1, -1, -1] = 0
        gb = g
    elif mutant == "drop_last_kstep_of_last_split":  # (kind 1: the last tile of the last split)
        g = g * (~(last & (sub == sub[last].max()))).double()[..., None]
        gb = g
    elif mutant == "drop_last_split":
        if plan["nsplit"] < 2:
            return None
        g = g * (~last).double()[..., None]
        gb = g
    elif mutant == "bias_misses_last_image":
        if not case.bias or n < 2:
            return None
        gb = g.clone()
        gb[-1] = 0
    elif mutant == "replicate_halo" and (ks == 1 or w == 1):
        return None
    R = Ref()
    R.flag_share = share
    gw = wgrad(g, a, ks, replicate_left=mutant == "replicate_halo")
    if mutant == "drop_corner_tap":
        if ks == 1 or h < ks // 2 + 1 or w < ks // 2 + 1:
            return None
        gw[:, :, 0, 0] = 0
    elif mutant == "drop_last_tap_group":
        if plan["n_tapgroups"] < 2:
            return None
        gw.view(gw.shape[0], gw.shape[1], -1)[:, :, (plan["n_tapgroups"] - 1) * T.WG_MAXT:] = 0
    elif mutant == "drop_last_channel_of_segment":
        gw[:, [sum(case.segs[:i + 1]) - 1 for i in range(len(case.segs))]] = 0
    elif mutant == "shift_segment_offset":
        if len(case.segs) < 2:
            return None
        off = case.segs[0]
        gw[:, off:] = torch.roll(gw[:, off:], 1, dims=1)
    A = wgrad(I.g.abs(), a_abs, ks)
    extra = wgrad(I.g.abs(), allow, ks) if allow is not None else torch.zeros_like(A)
    us = case.unscale
    R.w, R.A_w, extra = gw * us, A * us, extra * us
    R.b = R.A_b = R.tol_b = None
    if case.bias:
        R.b, R.A_b = gb.sum(dim=(0, 1, 2)) * us, I.g.abs().sum(dim=(0, 1, 2)) * us
    if case.accumulate:
        if mutant != "no_accumulate":
            R.w = R.w + I.prev_w
            R.b = R.b + I.prev_b if case.bias else None
        R.A_w = R.A_w + I.prev_w.abs()
        R.A_b = R.A_b + I.prev_b.abs() if case.bias else None
    elif mutant == "no_accumulate":
        return None
    R.k = K_ACC[T.family(case)]
    R.tol_w = R.k * U32 * R.A_w + extra + (n * h * w + 2) * 2.0 ** -149
    if case.bias:
        R.tol_b = R.k * U32 * R.A_b
    return R


def identical(ref, mut):
    """The mutation left this case's reference as it is (the taps it drops lie outside a small image ...): it does not apply."""
    return torch.equal(ref.w, mut.w) and (ref.b is None or torch.equal(ref.b, mut.b))


def told_apart(ref, mut):
    """Does the tolerance of `ref` tell the mutated reference from it (some element of grad_w or grad_b outside the bound)?"""
    out = bool(((mut.w - ref.w).abs() > ref.tol_w).any())
    if ref.b is not None:
        out = out or bool(((mut.b - ref.b).abs() > ref.tol_b).any())
    return out


# ------------------------------------------------------------------------------------------------- the sequential f32 chain
def chain_error(case, I, plan=None, budget=1 << 22):
    """Worst |chain - exact| / (2^-24 A) of one pixel-ordered f32 fmaf chain (acc = float32(acc + g_px a_px)) over the case's own operands
    rounded to f32, against the exact sum of the same products.  Every (co, ci) of the centre tap where the budget of multiply-adds
    allows; of a larger case the first and last channels on both sides."""
    plan = plan or T.plan(T.problem(case))
    a, _, _, _ = activated(case, I, plan["kind"])
    P = case.n * case.h * case.w
    G = I.g.reshape(P, -1).float().double()
    X = a.reshape(P, -1).float().double()
    lim = max(8, int(math.sqrt(budget / P)))
    if G.shape[1] > lim:
        G = torch.cat([G[:, :lim // 2], G[:, -lim // 2:]], dim=1)
    if X.shape[1] > lim:
        X = torch.cat([X[:, :lim // 2], X[:, -lim // 2:]], dim=1)
    acc = torch.zeros((G.shape[1], X.shape[1]), dtype=torch.float32)
    for p in range(P):
        acc = (acc.double() + G[p, :, None] * X[p, None, :]).float()  # (the product of two f32 is exact in f64)
    exact, A = G.t() @ X, G.abs().t() @ X.abs()
    return float(((acc.double() - exact).abs() / (U32 * A).clamp_min(1e-300)).max())


def measure_k_acc(cases, bf16=False, budget=1 << 22):
    worst = {}
    for c in cases:
        e = chain_error(c, make_inputs(c, bf16), None, budget)
        f = T.family(c)
        worst[f] = max(worst.get(f, 0.0), e)
    return worst


if __name__ == "__main__":
    for fam, e in sorted(measure_k_acc(T.CASES).items()):
        print(f"{fam:10s} worst chain error {e:.3f} x 2^-24 A   -> k_acc >= {K_MARGIN * e:.2f}   (recorded {K_ACC[fam]})")
