"""The cases of tests/test_gpu_predictor_sites.py and a plain-Python mirror of the host side of csrc/predictor.hip: the stack
geometry (pred_geo), the 3x3 layers (tile_layer), the channel blocking (tile_ct), the NP rule and the grids of tile_forward /
tile_bwd_layer / tile_bwd_stem, and the fused placement's LDS test (pred_fused_ok).  For a case the mirror names every launch of
the tiled placement: kernel family, template parameters, layer and block count -- the record cgen_predictor_tiled_plan reports.
tests/test_predictor_cases.py holds the table to the sweep over every width and resolution the ABI accepts."""
from collections import namedtuple

NORMAL, CATEGORICAL, BERNOULLI = 0, 1, 2
WIDTHS = (8, 16, 24, 32)
R_MIN, R_MAX = 8, 512
TCH = 8                 # channels staged per chunk by the 3x3 kernels; the stem stages 4
MAX_OUT = 16
HS_TOTAL = 576
PRED_LDS_MAX = 160 * 1024 - HS_TOTAL * 4 - 1024

# kernel families of a plan record
FWD, BWD, STEM_BWD, TAIL = 0, 1, 2, 3

Geo = namedtuple("Geo", "c r w s1 h1 pool p h2 h4 h6 a1 ap a2 a3 a4 a5 a6 used total")
Layer = namedtuple("Layer", "cin cout hin hout s src dst")
# one launch: family, K, S, NP, CT, flag (POOL of a forward conv, MODE of a data gradient, BWD of the tail), layer, blocks
Launch = namedtuple("Launch", "family K S NP CT flag layer blocks")
Head = namedtuple("Head", "kind nout ctx tanh_loc std_fixed width", defaults=(None,))
Case = namedtuple("Case", "tag C R width n heads")


def pred_geo(c, r, w):
    s1 = 2 if r > 64 else 1
    h1 = (r - 1) // s1 + 1
    pool = r > 32
    p = h1 // 2 if pool else h1
    h2 = (p - 1) // 2 + 1
    h4 = (h2 - 1) // 2 + 1
    h6 = (h4 - 1) // 2 + 1
    o = 0
    offs = []
    for n in (w * h1 * h1, w * p * p if pool else 0, 2 * w * h2 * h2, 2 * w * h2 * h2, 4 * w * h4 * h4, 4 * w * h4 * h4, 8 * w * h6 * h6):
        offs.append(o)
        o += n
    return Geo(c, r, w, s1, h1, pool, p, h2, h4, h6, *offs, o, (o + 3) // 4 * 4)


def tile_layer(g, L):
    w = g.w
    return {1: Layer(w, 2 * w, g.p, g.h2, 2, g.a1, g.a2), 2: Layer(2 * w, 2 * w, g.h2, g.h2, 1, g.a2, g.a3),
            3: Layer(2 * w, 4 * w, g.h2, g.h4, 2, g.a3, g.a4), 4: Layer(4 * w, 4 * w, g.h4, g.h4, 1, g.a4, g.a5),
            5: Layer(4 * w, 8 * w, g.h4, g.h6, 2, g.a5, g.a6)}[L]


def tile_ct(ch):
    return 8 if ch % 32 == 0 else 6 if ch % 24 == 0 else 4 if ch % 16 == 0 else 2


def _cdiv(a, b):
    return (a + b - 1) // b


def forward_plan(g, n, nheads, bwd=False):
    """The launches of tile_forward, in order: the stem, the five 3x3 layers, the tail."""
    pairs = n * nheads
    nt = _cdiv(g.h1, 16)
    out = [Launch(FWD, 7, g.s1, 2, tile_ct(g.w), 0, 0, pairs * nt * nt)]
    for L in range(1, 6):
        ly = tile_layer(g, L)
        ct, np_ = tile_ct(ly.cout), 2 if ly.hout > 12 else 1
        nt = _cdiv(ly.hout, 8 * np_)
        out.append(Launch(FWD, 3, ly.s, np_, ct, int(L == 1 and g.pool), L, pairs * (ly.cout // (4 * ct)) * nt * nt))
    out.append(Launch(TAIL, 0, 0, 0, 0, int(bwd), 6, pairs))
    return out


def backward_plan(g, n, nheads):
    """The launches of tile_backward, in order: the data gradients of layers 5 .. 1, then the stem's into dx."""
    pairs = n * nheads
    out = []
    for L in range(5, 0, -1):
        ly = tile_layer(g, L)
        ct = tile_ct(ly.cin)
        nt = _cdiv(_cdiv(ly.hin, ly.s), 8)
        out.append(Launch(BWD, 3, ly.s, 0, ct, int(L == 1 and g.pool), L, pairs * (ly.cin // (4 * ct)) * nt * nt))
    nt = _cdiv(_cdiv(g.r, g.s1), 16)
    out.append(Launch(STEM_BWD, 7, g.s1, 0, 0, 0, 0, n * nt * nt))
    return out


def plan(c, r, w, n, nheads):
    """What cgen_predictor_tiled_plan reports: the forward call's launches, then the data-gradient launches of the backward call."""
    g = pred_geo(c, r, w)
    return forward_plan(g, n, nheads) + backward_plan(g, n, nheads)


def instance(l):
    """The compiled instance a launch runs (the tail is not a conv instance)."""
    if l.family == FWD:
        return ("ptile_conv_fwd", l.K, l.S, l.NP, l.CT, bool(l.flag))
    if l.family == BWD:
        return ("ptile_conv_bwd", l.S, l.CT, l.flag)
    if l.family == STEM_BWD:
        return ("ptile_stem_bwd", l.S)
    return None


def tile_edge(g, l):
    """(extent, tile) in pixels of the plane a conv launch tiles: outputs of a forward conv, inputs of a data gradient."""
    if l.family == FWD:
        return (g.h1 if l.K == 7 else tile_layer(g, l.layer).hout), 8 * l.NP
    if l.family == BWD:
        return tile_layer(g, l.layer).hin, 8 * l.S
    return g.r, 16 * l.S


def edges(g, l):
    """Which tile edges a launch exercises: several tiles (interior halos), a ragged last tile, a plane smaller than one tile."""
    ext, t = tile_edge(g, l)
    e = set()
    if ext > t:
        e.add("multi")
        if ext % t:
            e.add("ragged")
    if ext < t:
        e.add("small")
    return e


def compiled_instances():
    """Every conv instance csrc/predictor.hip compiles (tests/test_predictor_tiled_abi.py counts them in the code object)."""
    s = {("ptile_conv_fwd", 7, st, 2, ct, False) for st in (1, 2) for ct in (2, 4, 6, 8)}
    s |= {("ptile_conv_fwd", 3, st, np_, ct, pool) for (st, pool) in ((1, False), (2, False), (2, True)) for np_ in (1, 2) for ct in (2, 4, 6, 8)}
    s |= {("ptile_conv_bwd", st, ct, mode) for (st, mode) in ((1, 0), (2, 0), (2, 1)) for ct in (2, 4, 6, 8)}
    s |= {("ptile_stem_bwd", 1), ("ptile_stem_bwd", 2)}
    return s


# reachable from no shape: a 3x3 layer has at least 16 output channels, and only layer 1 reads fewer than 16
UNREACHABLE = {("ptile_conv_fwd", 3, st, np_, 2, pool) for (st, pool) in ((1, False), (2, False), (2, True)) for np_ in (1, 2)} | {("ptile_conv_bwd", 1, 2, 0)}


def sweep():
    """instance -> {edge: smallest R that shows it} over every width and resolution the ABI accepts."""
    seen = {}
    for w in WIDTHS:
        for r in range(R_MIN, R_MAX + 1):
            g = pred_geo(1, r, w)
            for l in plan(1, r, w, 1, 1):
                k = instance(l)
                if k is None:
                    continue
                d = seen.setdefault(k, {})
                for e in edges(g, l):
                    d[e] = min(d.get(e, r), r)
    return seen


def lds_x(c, r):
    return (c * r * r + 3) // 4 * 4


def fused_ok(c, r, widths):
    """pred_fused_ok: no pool, and the image plus the largest head's stack fit the dynamic LDS."""
    if r > 32:
        return False
    return (lds_x(c, r) + max(pred_geo(c, r, w).total for w in widths)) * 4 <= PRED_LDS_MAX


def N(tanh=0, std=0.0, ctx=0, width=None):
    return Head(NORMAL, 2, ctx, tanh, std, width)


def Cat(nout, ctx=0, width=None):
    return Head(CATEGORICAL, nout, ctx, 0, 0.0, width)


def Bern(ctx=0, width=None):
    return Head(BERNOULLI, 1, ctx, 0, 0.0, width)


FOUR = [N(tanh=1, ctx=1), Cat(10), Bern(ctx=4), N(std=0.3)]
# R_CASE_MAX: the largest resolution a case may have (the suite's time); an edge the sweep first shows above it is named in
# test_predictor_cases.py, not covered
R_CASE_MAX = 140
CASES = [
    # the 13 shapes of the greedy cover of the 39 reachable instances
    Case("r8w8", 1, 8, 8, 2, [N()]),
    Case("r65w24", 1, 65, 24, 2, [Cat(3), Bern()]),
    Case("r50w16", 3, 50, 16, 2, [N(tanh=1), Cat(10, ctx=1)]),
    Case("r99w8", 1, 99, 8, 2, FOUR),
    Case("r25w24", 1, 25, 24, 1, [Bern()]),
    Case("r33w32", 1, 33, 32, 1, [N()]),
    Case("r8w24", 4, 8, 24, 3, [Cat(2)]),
    Case("r25w8", 3, 25, 8, 3, FOUR),
    Case("r33w8", 4, 33, 8, 2, [N(ctx=4), Bern()]),
    Case("r25w16", 1, 25, 16, 2, [N(tanh=1, ctx=1), Cat(4)]),
    Case("r50w24", 1, 50, 24, 1, [N(std=0.5)]),
    Case("r65w16", 1, 65, 16, 1, [Cat(16)]),
    Case("r65w32", 1, 65, 32, 1, [Bern(ctx=1)]),
    # the boundaries: the pool switches on above 32, the stem's stride above 64; odd h1 behind the pool (66 -> 33, 35 -> 35)
    Case("r32w8", 1, 32, 8, 2, [N(tanh=1, ctx=1), N(tanh=1), Cat(10)]),
    Case("r64w8", 3, 64, 8, 1, [Cat(10), Cat(3)]),
    Case("r66w16", 1, 66, 16, 2, [N(), Bern(ctx=1)]),
    Case("r35w24", 1, 35, 24, 2, [Bern(), Cat(5)]),
    Case("r35w8", 1, 35, 8, 1, [N(tanh=1)]),
    Case("r36w32", 1, 36, 32, 1, [Cat(3)]),
    # tile edges the shapes above leave out (test_predictor_cases.py names the instance and the edge if one is missing):
    # several 16-pixel tiles of a 3x3 layer need h2 > 16, i.e. R >= 131; a stem plane smaller than its tile needs R < 16
    Case("r131w24", 1, 131, 24, 1, [Bern()]),
    Case("r131w16", 1, 131, 16, 1, [N()]),
    Case("r131w8", 1, 131, 8, 1, [Cat(4)]),
    Case("r18w8", 1, 18, 8, 1, [N()]),
    Case("r19w24", 1, 19, 24, 1, [N()]),
    Case("r19w32", 1, 19, 32, 1, [Cat(2)]),
    Case("r9w16", 3, 9, 16, 2, [N(tanh=1)]),
    Case("r12w32", 1, 12, 32, 1, [Bern()]),
    # terms above 256: pred_sum_kernel's strided partials (n * nheads = 260 at the smallest image)
    Case("sum260", 1, 8, 8, 65, FOUR),
]
# workspace and fused placements only (pred_validate does not ask for equal widths; the tiled path does)
MIXED = [Case("mixed_r16", 1, 16, 8, 2, [N(width=8), Cat(3, ctx=1, width=16), Bern(width=8)]),
         Case("mixed_r40", 3, 40, 8, 2, [Bern(width=16), N(tanh=1, width=8)])]


def head_width(case, h):
    return h.width if h.width is not None else case.width


def by_tag(tag):
    return next(c for c in CASES + MIXED if c.tag == tag)
