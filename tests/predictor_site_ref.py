"""f64 layer-local references of csrc/predictor.hip (inference forward and input gradient of the anticausal CNN) for the cases of
tests/predictor_cases.py: the inputs of a case (drawn on the CPU from the case's tag, so that the GPU test and the CPU checks of
tests/test_predictor_cases.py see the same numbers), one reference per SITE computed from the operands AS STORED, its tolerance, the
mutants the tolerance has to tell from the reference, and the emulation of one sequential f32 fmaf chain from which the
accumulation constants are measured (`python tests/predictor_site_ref.py` prints the table).

After a forward call the workspace and tiled placements leave every site's post-activation in the workspace (pred_geo's layout:
a1, ap, a2 .. a6); after a backward call the same planes hold d loss / d pre-activation.  A site's reference is one layer applied
in f64 to the f32 planes the device itself stored for that layer's input, so that errors do not compound:

  forward   a_L = lrelu(conv(a_{L-1}) + b)          (layer 1 behind the pool: of the pooled a1 -- a selection, exact)
  tail      outs = fc3(lrelu(fc0([mean(a6), y])))   (feat and hid are not stored: one reference from a6 to outs)
  terms     pred_nll(outs as stored, obs)
  a6'       the tail's backward from the stored outs; fc0's LeakyReLU mask from the f64 hid (`hid_margin` says how far from 0)
  a_{L-1}'  = conv^T(a_L') * lrelu'(a_{L-1} of the forward snapshot); behind the pool, scattered to the first maximum of each
              window of the forward snapshot's a1, zero elsewhere, the uncovered row and column of an odd plane included
  dx        = sum over heads of conv^T(a1')
The LeakyReLU mask (post > 0; the derivative at exactly 0 is LEAK, as torch's) and the pool's argmax (first maximum in row-major
order) are taken from the device's own f32 planes, so no element is ill-conditioned and none is left out.

Tolerance per element: |got - ref| <= k 2^-24 A + floor.  A = the same layer on absolute values, bias included (LeakyReLU is
1-Lipschitz, a mask multiplies A by its value); floor = 2^-149, the smallest subnormal (a gradient that underflows).  k = K_ACC of
the family + one per further rounding (the bias add of the tiled kernels, the mask product, the mean's division).  K_ACC is
K_MARGIN = 4 times the worst error of ONE sequential f32 fmaf chain over each element's terms on every case's inputs, rounded up.
A site that is the composition of unstored steps (the tail) propagates: each step's bound plus |W| times the bound of its input.
pred_nll: k_nll 2^-24 M, M = the magnitudes of the term's summands (see `nll`), k_nll measured alike from the same formula in f32.
No constant comes from a GPU result.

LEAK is the kernel's 0.01f, i.e. the f32 value: the references and the whole-network autograd check use that slope."""
import math
import zlib

import torch
import torch.nn.functional as F

from predictor_cases import (BERNOULLI, CATEGORICAL, MAX_OUT, NORMAL, TCH, Case, Head, head_width, pred_geo, tile_ct, tile_layer)

U32 = 2.0 ** -24
TINY = 2.0 ** -149
K_MARGIN = 4
LEAK = float(torch.tensor(0.01, dtype=torch.float32))
EPS32 = float(torch.finfo(torch.float32).eps)
LOGIT_MAX = float(torch.tensor(15.942384719848633, dtype=torch.float32))
HALF_LOG_2PI = float(torch.tensor(0.91893853320467274, dtype=torch.float32))
# family -> K_MARGIN x the worst sequential-chain error measured by `python tests/predictor_site_ref.py` over every case
# (the measured worst in the comment, in units of 2^-24 A)
K_ACC = {
    "stem": 21.0,      # measured 5.030
    "fwd3": 31.0,      # measured 7.693
    "bwd3": 30.0,      # measured 7.488
    "stem_bwd": 27.0,  # measured 6.517
    "tail": 28.0,      # measured 6.815
}
K_NLL = 12.0           # measured 2.783
COEF = 2.5


class Inputs:
    pass


def _f32(t):
    return t.to(torch.float32)


HID_MARGIN_MIN = 4.0


def make_inputs(case, hot=True):
    """The inputs of a case from the first seed (the tag's, then + 1 ...) at which no fc0 pre-activation lies within HID_MARGIN_MIN
    times its forward bound of 0: fc0's LeakyReLU mask is not stored, the backward reference takes it from the f64 hid."""
    for salt in range(64):
        I = _make_inputs(case, hot, salt)
        if _hid_margin(case, I) > HID_MARGIN_MIN:
            break
    I.salt = salt
    return I


def _hid_margin(case, I):
    worst = math.inf
    for H in I.heads:
        g = pred_geo(case.C, case.R, H.width)
        a = lrelu(F.conv2d(I.x.double(), H.w[0].double(), H.b[0].double(), stride=g.s1, padding=3)).float().double()
        if g.pool:
            a = pool_fwd(a, g.p)
        for L in range(1, 6):
            a = lrelu(F.conv2d(a, H.w[L].double(), H.b[L].double(), stride=tile_layer(g, L).s, padding=1)).float().double()
        _, _, pre, t_pre = tail_fwd(H, a)
        worst = min(worst, float((pre.abs() / t_pre).min()))
    return worst


def _make_inputs(case, hot, salt):
    """x [n, C, R, R] in [-1, 1] and, per head, folded weights and biases drawn directly, context, observation; all f32.
    Planted: a flat patch (pooled cases: whole pool windows of the stem tie), a zero patch in the last image's corner under two
    stem channels of zero bias (pre-activation exactly 0), and in a multi-head case the last classifier head saturated (its
    fc.3 scaled by 1e3) next to unsaturated heads."""
    g = torch.Generator().manual_seed(zlib.crc32(case.tag.encode()) + salt)
    I = Inputs()
    n, C, R = case.n, case.C, case.R
    x = torch.rand((n, C, R, R), generator=g, dtype=torch.float64) * 2 - 1
    s1 = 2 if R > 64 else 1
    I.flat = None
    if R > 32:
        fp = 8 + 8 * s1
        x[0, :, 3:3 + fp, 3:3 + fp] = 0.5
        I.flat = (3, fp)
    zp = min(R, 12)
    x[n - 1, :, R - zp:, R - zp:] = 0.0
    I.x = _f32(x)
    I.coef = torch.tensor([COEF], dtype=torch.float32)
    I.heads = []
    classifiers = [i for i, h in enumerate(case.heads) if h.kind != NORMAL]
    I.hot = classifiers[-1] if (hot and len(case.heads) > 1 and classifiers) else None
    for hi, h in enumerate(case.heads):
        w = head_width(case, h)
        H = Inputs()
        H.head, H.width = h, w
        chans = [(C, w, 7), (w, 2 * w, 3), (2 * w, 2 * w, 3), (2 * w, 4 * w, 3), (4 * w, 4 * w, 3), (4 * w, 8 * w, 3)]
        H.w, H.b = [], []
        for ci, co, k in chans:
            H.w.append(_f32(torch.randn((co, ci, k, k), generator=g, dtype=torch.float64) * (1.6 / math.sqrt(ci * k * k))))
            H.b.append(_f32(torch.randn((co,), generator=g, dtype=torch.float64) * 0.1))
        H.b[0][:2] = 0.0
        nf = 8 * w
        H.w.append(_f32(torch.randn((nf, nf + h.ctx), generator=g, dtype=torch.float64) * (1.6 / math.sqrt(nf + h.ctx))))
        H.b.append(_f32(torch.randn((nf,), generator=g, dtype=torch.float64) * 0.5))
        H.w.append(_f32(torch.randn((h.nout, nf), generator=g, dtype=torch.float64) * (1.6 / math.sqrt(nf))))
        H.b.append(_f32(torch.randn((h.nout,), generator=g, dtype=torch.float64) * 0.5))
        if hi == I.hot:
            H.w[7] *= 1e3
            H.b[7] *= 1e3
        H.y = _f32(torch.randn((n, h.ctx), generator=g, dtype=torch.float64)) if h.ctx else None
        if h.kind == CATEGORICAL:
            H.obs = F.one_hot(torch.randint(0, h.nout, (n,), generator=g), h.nout).float()
        elif h.kind == BERNOULLI:
            H.obs = torch.randint(0, 2, (n, 1), generator=g).float()
        else:
            H.obs = _f32(torch.randn((n, 1), generator=g, dtype=torch.float64) * (0.5 if h.tanh_loc else 1.0))
        I.heads.append(H)
    return I


# ------------------------------------------------------------------------------------------------- pred_nll at its branch points
def _below(v):
    t = torch.tensor(v, dtype=torch.float32)
    return float(torch.nextafter(t, torch.tensor(-math.inf)))


def _above(v):
    t = torch.tensor(v, dtype=torch.float32)
    return float(torch.nextafter(t, torch.tensor(math.inf)))


# (head, exact outputs, obs rows of the two images, the branch the kernel's source takes)
NLL_POINTS = [
    (Head(NORMAL, 2, 0, 0, 0.0), (0.25, _below(20.0)), [[0.5], [-1.0]], "softplus"),
    (Head(NORMAL, 2, 0, 0, 0.0), (0.25, 20.0), [[0.5], [-1.0]], "softplus"),        # ls > 20 is false AT 20
    (Head(NORMAL, 2, 0, 0, 0.0), (0.25, _above(20.0)), [[0.5], [-1.0]], "linear"),
    (Head(NORMAL, 2, 0, 0, 0.0), (-1.5, -8.0), [[-1.5], [-1.4990234375]], "softplus"),  # a tiny scale; z = 0 and z large
    (Head(NORMAL, 2, 0, 1, 0.0), (4.0, 0.5), [[0.75], [-0.75]], "softplus"),         # tanh_loc near +1
    (Head(NORMAL, 2, 0, 1, 0.0), (-9.0, 0.5), [[0.75], [-1.0]], "softplus"),        # tanh_loc at -1 in f32
    (Head(NORMAL, 2, 0, 1, 0.25), (0.5, 32.0), [[0.25], [1.0]], "fixed"),           # std_fixed > 0: ls is not read
    (Head(NORMAL, 2, 0, 0, 2.0), (0.5, -4.0), [[0.25], [1.0]], "fixed"),
    (Head(BERNOULLI, 1, 0, 0, 0.0), (_below(LOGIT_MAX),), [[1.0], [0.0]], "inside"),
    (Head(BERNOULLI, 1, 0, 0, 0.0), (LOGIT_MAX,), [[1.0], [0.0]], "clamped"),       # z < L is false AT L: zero gradient
    (Head(BERNOULLI, 1, 0, 0, 0.0), (_above(LOGIT_MAX),), [[1.0], [0.0]], "clamped"),
    (Head(BERNOULLI, 1, 0, 0, 0.0), (64.0,), [[1.0], [0.0]], "clamped"),
    (Head(BERNOULLI, 1, 0, 0, 0.0), (-_below(LOGIT_MAX),), [[1.0], [0.0]], "inside"),
    (Head(BERNOULLI, 1, 0, 0, 0.0), (-LOGIT_MAX,), [[1.0], [0.0]], "clamped"),
    (Head(BERNOULLI, 1, 0, 0, 0.0), (-_above(LOGIT_MAX),), [[1.0], [0.0]], "clamped"),
    (Head(BERNOULLI, 1, 0, 0, 0.0), (0.0,), [[1.0], [0.0]], "inside"),
    (Head(CATEGORICAL, 2, 0, 0, 0.0), (0.0, 32.0), [[1.0, 0.0], [0.0, 1.0]], "sat"),  # pk = e^-32 << eps / pk = 1 - e^-32 >> 1 - eps
    (Head(CATEGORICAL, 3, 0, 0, 0.0), (0.5, -0.25, 1.0), [[0.5, 0.5, 0.0], [0.0, 1.0, 1.0]], "free"),  # tied obs: the first maximum
    (Head(CATEGORICAL, 3, 0, 0, 0.0), (2.0, 2.0, 2.0), [[0.0, 0.0, 0.0], [0.0, 0.0, 1.0]], "free"),    # an all-tied row: class 0
    (Head(CATEGORICAL, 16, 0, 0, 0.0), tuple(float(j % 5) - 2.0 for j in range(16)), [[0.0] * 15 + [1.0], [1.0] + [0.0] * 15], "free"),
]


def nll_cases():
    """The branch points, four heads to a call (C = 1, R = 8, width 8, two images)."""
    out = []
    for i in range(0, len(NLL_POINTS), 4):
        pts = NLL_POINTS[i:i + 4]
        out.append((Case("nll%d" % (i // 4), 1, 8, 8, 2, [p[0] for p in pts]), pts))
    return out


def make_nll_inputs(case, pts):
    """A zero last conv and ctx = 0 make feat exactly 0, so hid = lrelu(fc0's bias) exactly whatever fc0's weight; a signed one-hot
    fc.3 then makes the head outputs the chosen f32 values exactly.  The a6 planes after backward are still a non-zero linear image
    of d nll / d out through fc.3, fc0's weight and LEAK."""
    I = make_inputs(case, hot=False)
    for H, (h, outs, obs, _) in zip(I.heads, pts):
        H.w[5].zero_()
        H.b[5].zero_()
        H.w[7].zero_()
        H.b[7].zero_()
        for o, v in enumerate(outs):
            H.b[6][o] = abs(v) if v != 0 else 1.0
            H.w[7][o, o] = math.copysign(1.0, v) if v != 0 else 1.0
            H.b[7][o] = 0.0 if v != 0 else -1.0  # (an output of exactly 0 is 1 - 1, so that its gradient still flows)
        H.obs = torch.tensor(obs, dtype=torch.float32)
        H.exact_outs = torch.tensor(outs, dtype=torch.float32)
    return I


# ------------------------------------------------------------------------------------------------- pred_nll
def nll(h, o, obs, dt=torch.float64):
    """pred_nll restated with the kernel's own branches on the stored values: (term, d term / d o, M of the term, M of d, branch,
    margin), rows = samples.  `dt` = float32 evaluates the same formula in f32 (for k_nll).  M is the sum of the magnitudes of
    the summands, with |obs| + |loc| for the difference obs - loc and 1 + |o_j - m| for a softmax probability (the argument's
    rounding enters exp relatively).  margin: the relative distance of the categorical pk from its two clamps (the only branch
    decided by a COMPUTED comparison; inf elsewhere)."""
    o, obs = o.to(dt), obs.to(dt)
    n = o.shape[0]
    inf = torch.full((n,), math.inf, dtype=torch.float64)
    if h.kind == NORMAL:
        raw, ls = o[:, 0], o[:, 1]
        loc = torch.tanh(raw) if h.tanh_loc else raw
        if h.std_fixed > 0:
            sc = torch.full_like(ls, float(torch.tensor(h.std_fixed, dtype=torch.float32)))
            dsc = torch.zeros_like(ls)
            branch = ["fixed"] * n
        else:
            lin = ls > 20.0
            lsc = torch.where(lin, torch.zeros_like(ls), ls)
            sc = torch.where(lin, ls, torch.log1p(torch.exp(lsc)))
            dsc = torch.where(lin, torch.ones_like(ls), 1.0 / (1.0 + torch.exp(-lsc)))
            branch = ["linear" if b else "softplus" for b in lin.tolist()]
        z = (obs[:, 0] - loc) / sc
        za = (obs[:, 0].abs() + loc.abs()) / sc
        dloc = -z / sc
        d0 = dloc * (1.0 - loc * loc) if h.tanh_loc else dloc
        d1 = (1.0 - z * z) / sc * dsc
        term = 0.5 * z * z + torch.log(sc) + HALF_LOG_2PI
        M = 0.5 * za * za + torch.log(sc).abs() + HALF_LOG_2PI
        Md0 = za / sc * ((1.0 + loc * loc) if h.tanh_loc else 1.0)
        Md1 = (1.0 + za * za) / sc * dsc
        return term, torch.stack([d0, d1], 1), M, torch.stack([Md0, Md1], 1), branch, inf
    if h.kind == CATEGORICAL:
        k = (obs == obs.max(1, keepdim=True).values).to(torch.float64).mul(torch.arange(obs.shape[1], 0, -1, dtype=torch.float64)).argmax(1)
        m = o.max(1, keepdim=True).values
        e = torch.exp(o - m)
        s = e.sum(1, keepdim=True)
        p = e / s
        pk = p.gather(1, k[:, None])[:, 0]
        ok = (o - m).gather(1, k[:, None])[:, 0]
        lo, hi = pk < EPS32, pk > 1.0 - EPS32
        sat = lo | hi
        one = F.one_hot(k, o.shape[1]).to(dt)
        d = torch.where(sat[:, None], torch.zeros_like(p), p - one)
        term = torch.where(lo, torch.full_like(pk, -math.log(EPS32)), torch.where(hi, torch.full_like(pk, -math.log1p(-EPS32)), torch.log(s[:, 0]) - ok))
        M = torch.where(sat, term.abs(), torch.log(s[:, 0]).abs() + ok.abs() + 1.0)
        Md = torch.where(sat[:, None], torch.zeros_like(p), p * (1.0 + (o - m).abs()) + one)
        margin = torch.minimum((pk.double() / EPS32 - 1).abs(), ((1 - pk.double()) / EPS32 - 1).abs())
        return term, d, M, Md, ["sat" if b else "free" for b in sat.tolist()], margin
    z, v = o[:, 0], obs[:, 0]
    zc = z.clamp(-LOGIT_MAX, LOGIT_MAX)
    inside = (z > -LOGIT_MAX) & (z < LOGIT_MAX)
    sig = 1.0 / (1.0 + torch.exp(-zc))
    d = torch.where(inside, sig - v, torch.zeros_like(z))
    l1p = torch.log1p(torch.exp(-zc.abs()))
    term = zc.clamp_min(0) - zc * v + l1p
    M = zc.clamp_min(0) + (zc * v).abs() + l1p
    Md = torch.where(inside, sig + v.abs(), torch.zeros_like(z))
    return term, d[:, None], M, Md[:, None], ["inside" if b else "clamped" for b in inside.tolist()], inf


# ------------------------------------------------------------------------------------------------- sites
def lrelu(v):
    return torch.where(v > 0, v, LEAK * v)


def lrelu_d(post, wrong_side=False):
    return torch.where((post >= 0) if wrong_side else (post > 0), torch.ones_like(post), torch.full_like(post, LEAK))


_ORDER = torch.tensor([4.0, 3.0, 2.0, 1.0], dtype=torch.float64)


def pool_windows(a1, p):
    w = a1[..., :2 * p, :2 * p]
    return torch.stack([w[..., 0::2, 0::2], w[..., 0::2, 1::2], w[..., 1::2, 0::2], w[..., 1::2, 1::2]], -1)


def pool_argmax(a1, p, last=False):
    """The first (mutant: last) maximum of each 2 x 2 window in row-major order: (k, windows)."""
    win = pool_windows(a1, p)
    eq = (win == win.max(-1, keepdim=True).values).to(torch.float64)
    k = (eq * (_ORDER.flip(0) if last else _ORDER)).argmax(-1)
    return k, win


def pool_fwd(a1, p, last=False):
    k, win = pool_argmax(a1, p, last)
    return win.gather(-1, k[..., None])[..., 0]


def pool_bwd(a1_post, gp, p, last=False, wrong_side=False, keep_odd=False):
    """gp = d / d pooled plane -> d / d stem pre-activation: to the selected element times lrelu', zero elsewhere."""
    k, _ = pool_argmax(a1_post, p, last)
    out = a1_post.clone() if keep_odd else torch.zeros_like(a1_post)
    d = lrelu_d(a1_post, wrong_side)
    for e in range(4):
        ys, xs = slice(e >> 1, 2 * p, 2), slice(e & 1, 2 * p, 2)
        out[..., ys, xs] = torch.where(k == e, gp * d[..., ys, xs], torch.zeros_like(gp))
    return out


class Site:
    """What a reference needs to know of the kernel that writes a site: tile (pixels), channel group, staged chunk, and for the
    mutants' sake only -- the reference itself does not depend on them."""

    def __init__(self, name, family, K, S, tile, group, chunk, pool=False):
        self.name, self.family, self.K, self.S, self.tile, self.group, self.chunk, self.pool = name, family, K, S, tile, group, chunk, pool


def sites_of(g, placement):
    """site name -> Site for the forward convs ('a1' .. 'a6') and the data gradients ('g1' = into a1 .. 'g5' = into a5, 'dx')."""
    tiled = placement == "tiled"
    s = {"a1": Site("a1", "stem", 7, g.s1, 16 if tiled else None, tile_ct(g.w) if tiled else 8, 4 if tiled else 1)}
    for L in range(1, 6):
        ly = tile_layer(g, L)
        np_ = 2 if ly.hout > 12 else 1
        s["a%d" % (L + 1)] = Site("a%d" % (L + 1), "fwd3", 3, ly.s, 8 * np_ if tiled else None, tile_ct(ly.cout) if tiled else 8, TCH if tiled else 1,
                                  pool=L == 1 and g.pool)
        s["g%d" % L] = Site("g%d" % L, "bwd3", 3, ly.s, 8 * ly.s if tiled else None, tile_ct(ly.cin) if tiled else 8, TCH if tiled else 1,
                            pool=L == 1 and g.pool)
    s["dx"] = Site("dx", "stem_bwd", 7, g.s1, 16 * g.s1 if tiled else None, 1, TCH if tiled else 1)
    return s


def _drop_tile_edge(ref, tile, rows):
    """The last row (column) of every tile never written: what the NaN prefill would show; the mutant leaves zeros."""
    h = ref.shape[-1]
    idx = [i for i in range(h) if i % tile == tile - 1 or i == h - 1]
    out = ref.clone()
    if rows:
        out[..., idx, :] = 0
    else:
        out[..., idx] = 0
    return out


def conv_site(st, inp, w, b, mutant=None):
    """Forward conv + bias + LeakyReLU of one site from its stored input planes (f64 [n, ci, h, h]): (ref, A) or None where the
    mutant does not apply."""
    K, S, p = st.K, st.S, st.K // 2
    w, b = w.double(), b.double()
    wm, x = w, inp
    post = None
    if mutant == "corner_tap":
        wm = w.clone()
        wm[:, :, 0, 0] = 0
    elif mutant == "halo_replicate":
        x = F.pad(F.pad(inp, (p, 0, p, 0), mode="replicate"), (0, p, 0, p))
    elif mutant == "last_chunk":
        c0 = (w.shape[1] - 1) // st.chunk * st.chunk
        wm = w.clone()
        wm[:, c0:] = 0
    elif mutant == "parity":
        if S != 2:
            return None
        x = F.pad(inp, (0, 1, 0, 1))[..., 1:, 1:]
    elif mutant == "no_bias":
        b = torch.zeros_like(b)
    elif mutant in ("tile_row", "tile_col"):
        if st.tile is None:
            return None
    elif mutant == "group_channel":
        pass
    elif mutant is not None:
        return None
    pre = F.conv2d(x, wm, None, stride=S, padding=0 if mutant == "halo_replicate" else p) + b.view(1, -1, 1, 1)
    A = F.conv2d(inp.abs(), w.abs(), None, stride=S, padding=p) + b.abs().view(1, -1, 1, 1)
    post = lrelu(pre)
    if mutant in ("tile_row", "tile_col"):
        post = _drop_tile_edge(post, st.tile, mutant == "tile_row")
    if mutant == "group_channel":
        post = post.clone()
        post[:, st.group - 1::st.group] = 0
    return post, A


def _convT(g, w, K, S, hin):
    hout = g.shape[-1]
    return F.conv_transpose2d(g, w, None, stride=S, padding=K // 2, output_padding=hin - ((hout - 1) * S - 2 * (K // 2) + K))


def dgrad_site(st, gout, w, hin, mutant=None):
    """Data gradient of one conv from the stored d / d pre-activation planes of its output: (gi, A) before any mask, or None."""
    K, S = st.K, st.S
    w = w.double()
    wm = w
    if mutant == "corner_tap":
        wm = w.clone()
        wm[:, :, 0, 0] = 0
    elif mutant == "last_chunk":
        c0 = (w.shape[0] - 1) // st.chunk * st.chunk
        wm = w.clone()
        wm[c0:] = 0
    elif mutant == "halo_replicate":
        gp = F.pad(gout, (1, 0, 1, 0), mode="replicate")
        hout = gp.shape[-1]
        full = F.conv_transpose2d(gp, w, None, stride=S, padding=K // 2, output_padding=S - 1)
        gi = full[..., S:S + hin, S:S + hin]
        if gi.shape[-1] != hin:
            return None
        return gi, _convT(gout.abs(), w.abs(), K, S, hin)
    elif mutant == "parity":
        if S != 2:
            return None
        gi = _convT(gout, w, K, S, hin)
        return torch.roll(gi, (1, 1), (-2, -1)), _convT(gout.abs(), w.abs(), K, S, hin)
    elif mutant in ("tile_row", "tile_col"):
        if st.tile is None:
            return None
    elif mutant == "group_channel":
        pass
    elif mutant is not None:
        return None
    gi = _convT(gout, wm, K, S, hin)
    if mutant in ("tile_row", "tile_col"):
        gi = _drop_tile_edge(gi, st.tile, mutant == "tile_row")
    if mutant == "group_channel":
        gi = gi.clone()
        gi[:, st.group - 1::st.group] = 0
    return gi, _convT(gout.abs(), w.abs(), K, S, hin)


def tol_of(A, k):
    return k * U32 * A + TINY


def tail_fwd(H, a6, mutant=None):
    """outs from the stored a6 planes: (outs, tol, hid pre-activation, its tol).  Three unstored steps: the bound propagates."""
    k = K_ACC["tail"]
    n, nf, h6, _ = a6.shape
    hw6 = h6 * h6
    w6, b6, w7, b7 = H.w[6].double(), H.b[6].double(), H.w[7].double(), H.b[7].double()
    feat = a6.sum((-2, -1)) / (h6 if mutant == "mean_h6" else hw6)
    t_feat = tol_of(a6.abs().sum((-2, -1)) / hw6, k + 1)
    if H.y is not None:
        y = H.y.double()
        if mutant == "last_ctx":
            y = torch.cat([y[:, :-1], torch.zeros_like(y[:, -1:])], 1)
        feat = torch.cat([feat, y], 1)
        t_feat = torch.cat([t_feat, torch.zeros_like(y)], 1)
    elif mutant == "last_ctx":
        return None
    if mutant == "mean_h6" and h6 == 1:
        return None
    if mutant == "no_bias":
        b6 = torch.zeros_like(b6)
    elif mutant not in (None, "mean_h6", "last_ctx"):
        return None
    pre = feat @ w6.t() + b6
    t_pre = tol_of(feat.abs() @ w6.abs().t() + H.b[6].double().abs(), k + 1) + t_feat @ w6.abs().t()
    hid = lrelu(pre)
    outs = hid @ w7.t() + b7
    t_out = tol_of(hid.abs() @ w7.abs().t() + b7.abs(), k + 1) + t_pre @ w7.abs().t()
    return outs, t_out, pre, t_pre


def tail_bwd(H, a6_post, outs, coef, mutant=None):
    """The a6 planes after the backward's tail, from the forward snapshot's a6 and the stored outs: (a6', tol, hid margin).
    hid margin = the smallest |hid pre-activation| / its forward bound: fc0's mask is not stored, so it must be far above 1."""
    h = H.head
    k = K_ACC["tail"]
    n, nf, h6, _ = a6_post.shape
    hw6 = h6 * h6
    w6, w7 = H.w[6].double(), H.w[7].double()
    _, _, pre, t_pre = tail_fwd(H, a6_post)
    margin = float((pre.abs() / t_pre).min())
    _, d, _, Md, branch, _ = nll(h, outs, H.obs)
    if mutant == "saturated_contributes":
        if h.kind == NORMAL or not any(b in ("sat", "clamped") for b in branch):
            return None
        if h.kind == CATEGORICAL:
            o = outs.double()
            k_ = (H.obs.double() == H.obs.double().max(1, keepdim=True).values).to(torch.float64).mul(
                torch.arange(h.nout, 0, -1, dtype=torch.float64)).argmax(1)
            d = torch.softmax(o, 1) - F.one_hot(k_, h.nout).double()
        else:
            d = (torch.sigmoid(outs.double().clamp(-LOGIT_MAX, LOGIT_MAX)) - H.obs.double())
    elif mutant == "no_coef":
        coef = 1.0
    elif mutant == "lrelu_zero_side":
        pass
    elif mutant is not None:
        return None
    g0 = d * coef
    t_g0 = (K_NLL + 1) * U32 * Md * abs(COEF) + TINY
    mask_h = lrelu_d(lrelu(pre))
    ghid = (g0 @ w7) * mask_h
    t_ghid = (tol_of(g0.abs() @ w7.abs(), k + 1) + t_g0 @ w7.abs()) * mask_h
    gfeat = (ghid @ w6)[:, :nf] / hw6
    t_gfeat = (tol_of(ghid.abs() @ w6.abs(), k + 1) + t_ghid @ w6.abs())[:, :nf] / hw6
    m6 = lrelu_d(a6_post, wrong_side=mutant == "lrelu_zero_side")
    ref = gfeat[:, :, None, None] * m6
    tol = t_gfeat[:, :, None, None] * m6 + U32 * ref.abs() + TINY
    return ref, tol, margin


# ------------------------------------------------------------------------------------------------- one head, site by site
class Stored:
    """The planes a placement leaves behind for one head, as f64 tensors holding the stored f32 values: .fwd / .bwd map
    'a1', 'ap' (workspace placement, pooled cases), 'a2' .. 'a6' to [n, ch, h, h]; .outs [n, nout], .terms [n]."""

    def __init__(self):
        self.fwd, self.bwd, self.outs, self.terms = {}, {}, None, None


def forward_refs(case, I, hi, S, placement, mutant=None):
    """site -> (ref, tol) of the forward call of head `hi`, each from the planes of S.fwd that the site's kernel reads.
    Sites: a1, (ap), a2 .. a6, outs, terms.  A mutant returns only the sites it changes."""
    H = I.heads[hi]
    g = pred_geo(case.C, case.R, H.width)
    st = sites_of(g, placement)
    bias_k = 1 if placement == "tiled" else 0  # the tiled kernels add the bias after the chain, the others start the chain from it
    out = {}

    def put(name, r, k):
        if r is not None:
            out[name] = (r[0], tol_of(r[1], k))

    conv_mut = mutant if mutant in ("corner_tap", "halo_replicate", "last_chunk", "parity", "no_bias", "tile_row", "tile_col", "group_channel") else None
    if mutant is None or conv_mut:
        put("a1", conv_site(st["a1"], I.x.double(), H.w[0], H.b[0], conv_mut), K_ACC["stem"] + bias_k + 1)
    src = S.fwd["a1"]
    if g.pool:
        last = mutant == "pool_last_max"
        pooled = pool_fwd(S.fwd["a1"], g.p, last)
        if placement != "tiled":
            if mutant is None or last:
                out["ap"] = (pooled, torch.zeros_like(pooled))
            src = S.fwd["ap"]
        else:
            src = pooled
            if last:
                put("a2", conv_site(st["a2"], src, H.w[1], H.b[1]), K_ACC["fwd3"] + bias_k + 1)
    elif mutant == "pool_last_max":
        return out
    if mutant is None or conv_mut:
        for L in range(1, 6):
            name = "a%d" % (L + 1)
            put(name, conv_site(st[name], src, H.w[L], H.b[L], conv_mut), K_ACC["fwd3"] + bias_k + 1)
            src = S.fwd[name]
    if mutant in (None, "mean_h6", "last_ctx", "no_bias"):
        r = tail_fwd(H, S.fwd["a6"], mutant)
        if r is not None:
            out["outs"] = (r[0], r[1])
    if mutant is None:
        term, _, M, _, _, _ = nll(H.head, S.outs, H.obs)
        out["terms"] = (term, K_NLL * U32 * M)
    return out


def backward_refs(case, I, hi, S, placement, mutant=None):
    """site -> (ref, tol) of the planes after the backward call of head `hi`: a6 from the tail, a5 .. a1 (and ap) each from the
    stored gradient planes of the layer above and the forward snapshot's mask / argmax; 'dx1' = this head's share of dx."""
    H = I.heads[hi]
    g = pred_geo(case.C, case.R, H.width)
    st = sites_of(g, placement)
    out = {}
    if mutant in (None, "saturated_contributes", "no_coef", "lrelu_zero_side"):
        r = tail_bwd(H, S.fwd["a6"], S.outs, COEF, mutant)
        if r is not None:
            out["a6"] = (r[0], r[1])
            out["hid_margin"] = r[2]
    dg_mut = mutant if mutant in ("corner_tap", "halo_replicate", "last_chunk", "parity", "tile_row", "tile_col", "group_channel") else None
    wrong = mutant == "lrelu_zero_side"
    pool_mut = mutant in ("pool_last_max", "odd_not_zeroed")
    if mutant is None or dg_mut or wrong or pool_mut:
        for L in range(5, 0, -1):
            ly = tile_layer(g, L)
            dst = "a%d" % L
            pooled = L == 1 and g.pool
            if pool_mut and not pooled:
                continue
            r = dgrad_site(st["g%d" % L], S.bwd["a%d" % (L + 1)], H.w[L], ly.hin, dg_mut)
            if r is None:
                continue
            gi, A = r
            k = K_ACC["bwd3"] + 1
            if not pooled:
                m = lrelu_d(S.fwd[dst], wrong)
                out[dst] = (gi * m, tol_of(A * m, k))
                continue
            if placement != "tiled" and not pool_mut:
                out["ap"] = (gi, tol_of(A, K_ACC["bwd3"]))
                gi = S.bwd["ap"]  # (maxpool_bwd reads the stored plane)
                A = gi.abs()
                k = 1
            elif placement != "tiled":
                gi = S.bwd["ap"]
                A, k = gi.abs(), 1
            if mutant == "odd_not_zeroed" and g.h1 == 2 * g.p:
                continue
            ref = pool_bwd(S.fwd["a1"], gi, g.p, last=mutant == "pool_last_max", wrong_side=wrong, keep_odd=mutant == "odd_not_zeroed")
            Asc = pool_bwd(S.fwd["a1"], A, g.p).abs()
            out["a1"] = (ref, tol_of(Asc, k))
    if mutant is None or dg_mut:
        r = dgrad_site(st["dx"], S.bwd["a1"], H.w[0], case.R, dg_mut if dg_mut != "group_channel" else None)
        if r is not None and not (dg_mut == "group_channel"):
            out["dx1"] = (r[0], r[1])  # (ref, A): summed over heads by dx_ref
    return out


def dx_ref(parts, drop_last=False):
    """dx = the heads' shares added in head order: (ref, tol) from the per-head (gi, A) of backward_refs' 'dx1'."""
    use = parts[:-1] if drop_last else parts
    ref = sum(p[0] for p in use) if use else torch.zeros_like(parts[0][0])
    A = sum(p[1] for p in parts)
    return ref, tol_of(A, K_ACC["stem_bwd"] + len(parts))


def simulate(case, I, placement, round32=True):
    """The planes a correct device would store, by chaining the local references (each site rounded to f32 when `round32`):
    one Stored per head, and dx.  The CPU tests use it as the 'stored operands'; the GPU test never does."""
    rnd = (lambda t: t.float().double()) if round32 else (lambda t: t)
    stored, parts = [], []
    for hi, H in enumerate(I.heads):
        g = pred_geo(case.C, case.R, H.width)
        st = sites_of(g, placement)
        S = Stored()
        S.fwd["a1"] = rnd(conv_site(st["a1"], I.x.double(), H.w[0], H.b[0])[0])
        src = S.fwd["a1"]
        if g.pool:
            src = pool_fwd(src, g.p)
            if placement != "tiled":
                S.fwd["ap"] = src
        for L in range(1, 6):
            name = "a%d" % (L + 1)
            S.fwd[name] = src = rnd(conv_site(st[name], src, H.w[L], H.b[L])[0])
        S.outs = rnd(tail_fwd(H, S.fwd["a6"])[0])
        S.terms = rnd(nll(H.head, S.outs, H.obs)[0])
        S.bwd["a6"] = rnd(tail_bwd(H, S.fwd["a6"], S.outs, COEF)[0])
        for L in range(5, 0, -1):
            ly = tile_layer(g, L)
            gi = dgrad_site(st["g%d" % L], S.bwd["a%d" % (L + 1)], H.w[L], ly.hin)[0]
            if L == 1 and g.pool:
                gi = rnd(gi)
                if placement != "tiled":
                    S.bwd["ap"] = gi
                S.bwd["a1"] = rnd(pool_bwd(S.fwd["a1"], gi, g.p))
            else:
                S.bwd["a%d" % L] = rnd(gi * lrelu_d(S.fwd["a%d" % L]))
        parts.append(dgrad_site(st["dx"], S.bwd["a1"], H.w[0], case.R))
        stored.append(S)
    return stored, rnd(dx_ref(parts)[0])


MUTANTS = ("corner_tap", "halo_replicate", "tile_row", "tile_col", "group_channel", "last_chunk", "parity", "pool_last_max",
           "odd_not_zeroed", "lrelu_zero_side", "no_bias", "mean_h6", "last_ctx", "last_head", "no_coef", "saturated_contributes")


# ------------------------------------------------------------------------------------------------- whole network, for autograd
def network_nll(case, I, x):
    """sum over heads and samples of -log p through torch ops and tests/predictor_ref.py's likelihoods (torch.distributions), f64;
    x may require grad.  The slope is the kernel's f32 LEAK."""
    from predictor_ref import bernoulli_nll, categorical_nll, normal_nll

    total, outs = 0.0, []
    for H in I.heads:
        h = H.head
        g = pred_geo(case.C, case.R, H.width)
        a = F.leaky_relu(F.conv2d(x, H.w[0].double(), H.b[0].double(), stride=g.s1, padding=3), LEAK)
        if g.pool:
            a = F.max_pool2d(a, 2, 2)
        for L in range(1, 6):
            a = F.leaky_relu(F.conv2d(a, H.w[L].double(), H.b[L].double(), stride=tile_layer(g, L).s, padding=1), LEAK)
        f = a.mean((-2, -1))
        if H.y is not None:
            f = torch.cat([f, H.y.double()], 1)
        o = F.linear(F.leaky_relu(F.linear(f, H.w[6].double(), H.b[6].double()), LEAK), H.w[7].double(), H.b[7].double())
        outs.append(o)
        if h.kind == NORMAL:
            total = total + normal_nll(o, H.obs.double(), bool(h.tanh_loc), float(torch.tensor(h.std_fixed, dtype=torch.float32)))
        elif h.kind == CATEGORICAL:
            total = total + categorical_nll(o, H.obs.double())
        else:
            total = total + bernoulli_nll(o, H.obs.double())
    return total, outs


# ------------------------------------------------------------------------------------------------- the sequential f32 chain
def _chain(cols, wm, start=None, budget=1 << 22, seed=0):
    """Worst |chain - exact| / (2^-24 A) of acc = float32(acc + cols[:, k] * wm[k]) over k, rows of cols = elements."""
    P, L = cols.shape
    oc = wm.shape[1]
    S = max(1, min(P, budget // max(1, L * oc)))
    if S < P:
        pick = torch.randperm(P, generator=torch.Generator().manual_seed(seed))[:S]
        cols = cols[pick]
    acc = torch.zeros((cols.shape[0], oc), dtype=torch.float32) if start is None else start.float().expand(cols.shape[0], oc).clone()
    for k in range(L):
        acc = (acc.double() + cols[:, k:k + 1] * wm[k:k + 1]).float()
    exact = cols @ wm + (0 if start is None else start.double())
    A = cols.abs() @ wm.abs() + (0 if start is None else start.double().abs())
    return float(((acc.double() - exact).abs() / (U32 * A).clamp_min(1e-300)).max())


def _cols(x, K, S, pad):
    n, c, h, _ = x.shape
    u = F.unfold(x, K, padding=pad, stride=S)  # [n, c K K, P]
    return u.transpose(1, 2).reshape(-1, c * K * K)


def measure(cases, budget=1 << 21):
    """family -> worst chain error over the cases' own (simulated, f32-rounded) operands; 'nll' -> worst f32-formula error / (u M)."""
    worst = {k: 0.0 for k in list(K_ACC) + ["nll"]}

    def up(f, e):
        worst[f] = max(worst[f], e)

    for case, I in cases:
        stored, _ = simulate(case, I, "tiled" if len({H.width for H in I.heads}) == 1 else "workspace")
        for H, S in zip(I.heads, stored):
            g = pred_geo(case.C, case.R, H.width)
            up("stem", _chain(_cols(I.x.double(), 7, g.s1, 3), H.w[0].double().reshape(H.width, -1).t(), H.b[0][None], budget))
            src = pool_fwd(S.fwd["a1"], g.p) if g.pool else S.fwd["a1"]
            for L in range(1, 6):
                ly = tile_layer(g, L)
                up("fwd3", _chain(_cols(src, 3, ly.s, 1), H.w[L].double().reshape(ly.cout, -1).t(), H.b[L][None], budget))
                src = S.fwd["a%d" % (L + 1)]
                # data gradient: the transposed conv as a conv of the zero-stuffed gradient with the flipped, transposed weight
                go = S.bwd["a%d" % (L + 1)]
                z = torch.zeros(go.shape[0], go.shape[1], (go.shape[2] - 1) * ly.s + 1, (go.shape[3] - 1) * ly.s + 1, dtype=torch.float64)
                z[..., ::ly.s, ::ly.s] = go
                z = F.pad(z, (0, ly.hin - z.shape[-1], 0, ly.hin - z.shape[-1])) if z.shape[-1] < ly.hin else z
                wt = H.w[L].double().flip(2, 3).transpose(0, 1).reshape(ly.cin, -1).t()
                up("bwd3", _chain(_cols(z, 3, 1, 1), wt, None, budget))
            go = S.bwd["a1"]
            z = torch.zeros(go.shape[0], go.shape[1], (go.shape[2] - 1) * g.s1 + 1, (go.shape[3] - 1) * g.s1 + 1, dtype=torch.float64)
            z[..., ::g.s1, ::g.s1] = go
            z = F.pad(z, (0, case.R - z.shape[-1], 0, case.R - z.shape[-1])) if z.shape[-1] < case.R else z
            up("stem_bwd", _chain(_cols(z, 7, 1, 3), H.w[0].double().flip(2, 3).transpose(0, 1).reshape(case.C, -1).t(), None, budget))
            a6 = S.fwd["a6"]
            nf, hw6 = a6.shape[1], a6.shape[2] * a6.shape[3]
            up("tail", _chain(a6.reshape(-1, hw6), torch.ones((hw6, 1), dtype=torch.float64), None, budget))
            feat = a6.mean((-2, -1)).float().double()
            if H.y is not None:
                feat = torch.cat([feat, H.y.double()], 1)
            up("tail", _chain(feat, H.w[6].double().t(), H.b[6][None], budget))
            hid = lrelu(feat @ H.w[6].double().t() + H.b[6].double()).float().double()
            up("tail", _chain(hid, H.w[7].double().t(), H.b[7][None], budget))
            t64, d64, M, Md, _, _ = nll(H.head, S.outs, H.obs)
            t32, d32, _, _, _, _ = nll(H.head, S.outs, H.obs, torch.float32)
            up("nll", float(((t32.double() - t64).abs() / (U32 * M).clamp_min(1e-300)).max()))
            ok = Md > 0
            if ok.any():
                up("nll", float(((d32.double() - d64).abs()[ok] / (U32 * Md[ok])).max()))
    return worst


def all_inputs():
    from predictor_cases import CASES, MIXED

    out = [(c, make_inputs(c)) for c in CASES + MIXED]
    out += [(c, make_nll_inputs(c, pts)) for c, pts in nll_cases()]
    return out


if __name__ == "__main__":
    w = measure(all_inputs())
    for fam in K_ACC:
        print(f"{fam:9s} worst chain error {w[fam]:.3f} x 2^-24 A   -> k_acc >= {K_MARGIN * w[fam]:.2f}   (recorded {K_ACC[fam]})")
    print(f"{'nll':9s} worst f32-formula error {w['nll']:.3f} x 2^-24 M -> k_nll >= {K_MARGIN * w['nll']:.2f}   (recorded {K_NLL})")
