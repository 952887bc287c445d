"""The case table of the fused light Block's single launch (cgen_block3), shared by tests/test_block_cases.py (no GPU) and
tests/test_gpu_block3_f64.py: shapes, layouts, the argument record on given addresses, and the instance key cgen_block3_plan must
name for each case.

A case describes the FORWARD Block  cat(segs) -> b -> co  and a direction:
  fwd    seg = the segments, mid = the bottleneck (b), one output of co channels (+ bias, res1, remainder planes);
  dgrad  seg[0] = grad_out (co channels), mid = grad(bottleneck), mid_aux = the forward bottleneck, one output per differentiable
         segment k (`rg`): out.c = segs[k], aux = the forward segment, res1 = the gradient accumulated so far (or none).
A segment whose width is no multiple of 8 is the parents: spatially constant (strides 0, as engine.from_parents makes it), zero padded
to 8 through cgen_view.cpad; it never wants a gradient.

Instance keys, as cgen_block3_plan reports them (out[0 .. 6]):
  ("tile", PRE, NB, NPG, SM, TH, REM)    blk3_kernel<PRE, NB, NPG, SM, TH, REM>
  ("small", PRE)                         blk3s_kernel<PRE>
  ("rows", PRE, NCH, NB, RES, PROJ)      blk3r_kernel<PRE, NCH, NB, RES, PROJ> (NR = 1)

Layouts (`layout`): how every view but the parents sits in its parent tensor --
  "dense"  the parent is the view;
  "chan"   a channel slice: the parent is 16 channels wider, the view starts at channel 8;
  "win"    a window: the parent has one more image, two more rows, three more columns and 8 more channels, the view starts at its
           origin.  Everything of a parent that is not the view is NaN (tests/gpu_views.Arena.place)."""
import ctypes as C

from causal_gen_amd import _lib

PLAN_INTS = 24
KINDS = ("tile", "small", "rows")
FAKE = 1 << 20


class Case:
    dt = "h16"  # (the fused Block is a 16-bit kernel: tests/gpu_views.Arena reads this)

    def __init__(self, name, dir, n, h, w, segs, b, co, rg=None, bias="both", res1=None, rem=False, a16=False, down=False, layout="dense",
                 key=None, about=None):
        self.name, self.dir, self.n, self.h, self.w = name, dir, n, h, w
        self.segs, self.b, self.co = list(segs), b, co
        self.rg = list(rg) if rg is not None else [int(c % 8 == 0) for c in segs]
        self.bias = bias      # forward: "both", "a" (o[0].bias NULL), "o" (bias_a NULL), "none"; the down Block's projection bias rides with "o"
        self.res1 = res1      # None, "own", "alias" (forward: res1 IS seg[0])
        self.rem = rem        # forward: res1 and out are (hi, remainder plane) pairs
        self.a16 = a16        # the 16-row image of the first conv is given (w_a16)
        self.down = down      # the encoder's down Block: projection (+ 2x2 pooling forward)
        self.layout = layout
        self.key = key
        self.about = about or {}  # plan values the case is about, by name (PLAN_FIELDS)
        assert dir in ("fwd", "dgrad") and layout in ("dense", "chan", "win")
        assert all(not r or c % 8 == 0 for c, r in zip(self.segs, self.rg))

    def id(self):
        return f"{self.dir}-{self.name}"

    __repr__ = id

    @property
    def dsegs(self):
        return [k for k, r in enumerate(self.rg) if r]

    @property
    def nout(self):
        return 1 if self.dir == "fwd" else len(self.dsegs)

    @property
    def out_hw(self):
        return (self.h // 2, self.w // 2) if (self.down and self.dir == "fwd") else (self.h, self.w)

    def seg_off(self, k):
        return sum(self.segs[:k])

    def family(self):
        return self.key[0]


def cp8(c):
    return -(-c // 8) * 8


def parent_shape(case, shape):
    """(parent shape, channel offset) of a view of `shape` = (n, h, w, c) in the case's layout."""
    n, h, w, c = shape
    c8 = cp8(c)
    if case.layout == "chan":
        return (n, h, w, c8 + 16), 8
    if case.layout == "win":
        return (n + 1, h + 2, w + 3, c8 + 8), 0
    return (n, h, w, c8), 0


def view_of(case, ptr, shape):
    """The cgen_view of a tensor of `shape` whose first element is at `ptr`, in the case's layout (the parents: strides 0)."""
    n, h, w, c = shape
    if c % 8:
        return _lib.View(ptr, cp8(c), 0, 0, c, cp8(c))
    (pn, ph, pw, pc), _ = parent_shape(case, shape)
    return _lib.View(ptr, ph * pw * pc, pw * pc, pc, c, 0)


def proj_krow(c):
    """Row stride of the 1x1 projection's image (cgen_weight_prep modes 0 / 1): ceil32(ceil8(K)) + 32."""
    return -(-cp8(c) // 32) * 32 + 32


def args(case, ptr=None):
    """cgen_block3_args of the case.  ptr: role -> device address ("s0" .., "mid", "mid_aux", "out0" .., "aux0" .., "res0" .., "w_a", "w_a16",
    "bias_a", "w0" .., "bias0", "w_proj", "bias_proj", and "rem_out" / "rem_res": byte offsets of the remainder planes); None: aligned
    stand-ins (the planner is host code and dereferences nothing)."""
    P = (lambda k, d=FAKE: ptr[k]) if ptr is not None else (lambda k, d=FAKE: d)
    n, h, w = case.n, case.h, case.w
    a = _lib.Block3Args()
    fwd = case.dir == "fwd"
    a.dtype, a.n, a.h, a.w, a.nout, a.pre_act = _lib.F16, n, h, w, case.nout, int(fwd)
    a.w_a = P("w_a")
    a.w_a16 = P("w_a16") if case.a16 else None
    a.mid = view_of(case, P("mid"), (n, h, w, case.b))
    if fwd:
        a.nseg = len(case.segs)
        for k, c in enumerate(case.segs):
            a.seg[k] = view_of(case, P(f"s{k}"), (n, h, w, c))
        a.bias_a = P("bias_a") if case.bias in ("both", "a") else None
        a.mid_aux = _lib.NULL_VIEW
        o = a.o[0]
        o.w, o.bias = P("w0"), (P("bias0") if case.bias in ("both", "o") else None)
        ho, wo = case.out_hw
        o.out, o.aux = view_of(case, P("out0"), (n, ho, wo, case.co)), _lib.NULL_VIEW
        if case.res1 == "alias":
            o.res1 = a.seg[0]
        elif case.res1 == "own":
            o.res1 = view_of(case, P("res0"), (n, h, w, case.co))
        else:
            o.res1 = _lib.NULL_VIEW
        if case.rem:
            o.out_rem, o.res1_rem = P("rem_out", 1 << 24), P("rem_res", 1 << 24)
        if case.down:
            a.w_proj, a.proj_krow, a.pool = P("w_proj"), proj_krow(case.segs[0]), 2
            a.bias_proj = P("bias_proj") if case.bias in ("both", "o") else None
    else:
        a.nseg = 1
        a.seg[0] = view_of(case, P("s0"), (n, h, w, case.co))
        a.bias_a = None
        a.mid_aux = view_of(case, P("mid_aux"), (n, h, w, case.b))
        for j, k in enumerate(case.dsegs):
            o = a.o[j]
            o.w, o.bias = P(f"w{j}"), None
            o.out = view_of(case, P(f"out{j}"), (n, h, w, case.segs[k]))
            o.aux = view_of(case, P(f"aux{j}"), (n, h, w, case.segs[k]))
            o.res1 = view_of(case, P(f"res{j}"), (n, h, w, case.segs[k])) if case.res1 else _lib.NULL_VIEW
        if case.down:
            a.w_proj, a.proj_krow, a.pool = P("w_proj"), proj_krow(case.co), 0
    return a


PLAN_FIELDS = {"ns": 7, "wb_persist": 8, "grid": 9, "ntiles": 10, "s_rows": 11, "s_strips": 12, "s_nmb": 13, "r_rs": 14, "r_sx": 15, "r_sy": 16,
               "r_res_tile": 17, "lds": 18}


def key_of(out):
    kind = KINDS[out[0]]
    if kind == "tile":
        return ("tile",) + tuple(out[1:7])
    if kind == "small":
        return ("small", out[1])
    assert out[6] == 1  # (NR: no two-round instance is served)
    return ("rows",) + tuple(out[1:6])


def plan(lib, a):
    """(what cgen_block3_supported answers, instance key or None, plan values by name)."""
    out = (C.c_int32 * PLAN_INTS)()
    ok = lib.block3_plan(C.byref(a), out)
    if not ok:
        return 0, None, {}
    return ok, key_of(tuple(out)), {k: out[i] for k, i in PLAN_FIELDS.items()}


# ------------------------------------------------------------------------------------------------- the reachability sweep
def sweep_records():
    """A few thousand argument records over n, h, w, segments, b, co, nout, res1, remainder planes, w_a16 and the down fields: every
    value of every axis at which b3_fill / b3_plan take another branch."""
    shapes = [(1, 4, 4), (2, 6, 6), (3, 12, 12), (2, 14, 14), (1, 64, 14), (1, 65, 14), (2, 20, 28), (2, 24, 48), (1, 16, 48), (2, 18, 70), (2, 96, 96),
              (11, 48, 128), (5, 48, 128), (3, 15, 16), (1, 3, 16), (33, 16, 256)]
    seg_sets = [[32], [64], [96], [128], [24], [40], [32, 32], [24, 4, 40], [64, 4], [96, 4, 96], [160], [16]]
    recs = []
    for n, h, w in shapes:
        for segs in seg_sets:
            for b in (8, 16, 24, 32, 40, 64):
                for co in (24, 32, 64, 72, 96, 160, 232):
                    for d in ("fwd", "dgrad"):
                        for res1 in (None, "own", "alias"):
                            if res1 == "alias" and (d == "dgrad" or co != segs[0]):
                                continue
                            for a16 in (False, True):
                                for extra in ("", "rem", "down"):
                                    if extra == "rem" and (d == "dgrad" or not res1):
                                        continue
                                    if extra == "down" and not (a16 and len(segs) == 1):
                                        continue
                                    recs.append(Case("sweep", d, n, h, w, segs, b, co, res1=res1, rem=extra == "rem", a16=a16, down=extra == "down"))
    return recs


def T(*a, **k):
    return Case(*a, **k)


# One case (at least) per instance the dispatch can reach -- tests/test_block_cases.py holds the set of keys below to the set a sweep of
# cgen_block3_plan reaches -- then the conditions of b3_plan / b3_fill a case can be "about" (`about`: the plan values, asserted on the
# CPU).  Names: t<NB><NPG> the tile kernel's instances ("-sm" streaming, "-th12" twelve-row tiles, "-rem" remainder planes), s-* the
# small-image kernel (strips of s_rows rows; a 1-row strip is only ever the LAST one: 64 / w - 2 >= 2 for w <= 14), r<c>-<b>-* the
# row-streaming kernel (strips of 32 columns x r_rs rows in bands of four).  Shapes are the smallest that reach the condition: ragged
# in H and W (20 x 28, 12 x 40, 17 x 33, 9 x 20 against 8 x 16 tiles), 11 x 48 x 128 = 528 eight-row tiles for the twelve-row tile,
# 172 x 20 x 16 = 516 tiles of which every third is ragged for a persistent workgroup (workgroup 2 walks tile 2, four rows, then
# tile 514, a full one).
CASES = [
    T("t11", "fwd", 2, 20, 28, [24, 4, 40], 8, 32, key=('tile', 1, 1, 1, 0, 8, 0), about=dict(ns=3, wb_persist=0, grid=12, ntiles=12)),
    T("t11-rem", "fwd", 3, 12, 40, [40], 8, 32, bias='a', res1='own', rem=True, layout='chan', key=('tile', 1, 1, 1, 0, 8, 1), about=dict(ns=2, wb_persist=1, grid=18, ntiles=18)),
    T("t11-sm", "fwd", 1, 17, 33, [32], 8, 32, bias='o', res1='own', layout='win', key=('tile', 1, 1, 1, 1, 8, 0), about=dict(ns=2, wb_persist=1, grid=9, ntiles=9)),
    T("t12", "fwd", 2, 9, 20, [24, 4, 40], 8, 64, bias='none', key=('tile', 1, 1, 2, 0, 8, 0), about=dict(ns=3, wb_persist=0, grid=8, ntiles=8)),
    T("t12-rem", "fwd", 2, 20, 28, [96, 4, 96], 8, 64, res1='own', rem=True, layout='chan', key=('tile', 1, 1, 2, 0, 8, 1), about=dict(ns=3, wb_persist=0, grid=12, ntiles=12)),
    T("t12-sm", "fwd", 3, 12, 40, [24], 8, 64, bias='a', res1='own', layout='win', key=('tile', 1, 1, 2, 1, 8, 0), about=dict(ns=2, wb_persist=1, grid=18, ntiles=18)),
    T("t14", "fwd", 1, 17, 33, [96], 8, 96, bias='o', key=('tile', 1, 1, 4, 0, 8, 0), about=dict(ns=3, wb_persist=0, grid=9, ntiles=9)),
    T("t14-rem", "fwd", 2, 9, 20, [24, 4], 8, 96, bias='none', res1='own', rem=True, layout='chan', key=('tile', 1, 1, 4, 0, 8, 1), about=dict(ns=2, wb_persist=0, grid=8, ntiles=8)),
    T("t14-th12", "fwd", 11, 48, 128, [8], 8, 72, res1='own', layout='win', key=('tile', 1, 1, 4, 0, 12, 0), about=dict(ns=2, wb_persist=0, grid=352, ntiles=352)),
    T("t14-th12-rem", "fwd", 11, 48, 128, [16], 8, 72, bias='a', res1='own', rem=True, key=('tile', 1, 1, 4, 0, 12, 1), about=dict(ns=2, wb_persist=0, grid=352, ntiles=352)),
    T("t21", "fwd", 2, 20, 28, [40], 16, 24, bias='o', layout='chan', key=('tile', 1, 2, 1, 0, 8, 0), about=dict(ns=2, wb_persist=1, grid=12, ntiles=12)),
    T("t21-rem", "fwd", 3, 12, 40, [96, 4, 96], 16, 24, bias='none', res1='own', rem=True, layout='win', key=('tile', 1, 2, 1, 0, 8, 1), about=dict(ns=3, wb_persist=0, grid=18, ntiles=18)),
    T("t21-sm", "fwd", 1, 17, 33, [24], 16, 24, res1='own', key=('tile', 1, 2, 1, 1, 8, 0), about=dict(ns=2, wb_persist=1, grid=9, ntiles=9)),
    T("t22", "fwd", 2, 9, 20, [40], 16, 40, bias='a', layout='chan', key=('tile', 1, 2, 2, 0, 8, 0), about=dict(ns=2, wb_persist=1, grid=8, ntiles=8)),
    T("t22-rem", "fwd", 2, 20, 28, [32], 16, 40, bias='o', res1='own', rem=True, layout='win', key=('tile', 1, 2, 2, 0, 8, 1), about=dict(ns=2, wb_persist=1, grid=12, ntiles=12)),
    T("t22-sm", "fwd", 3, 12, 40, [16], 16, 40, bias='none', res1='own', key=('tile', 1, 2, 2, 1, 8, 0), about=dict(ns=2, wb_persist=1, grid=18, ntiles=18)),
    T("t24", "fwd", 1, 17, 33, [24, 4, 40], 16, 160, layout='chan', key=('tile', 1, 2, 4, 0, 8, 0), about=dict(ns=3, wb_persist=0, grid=9, ntiles=9)),
    T("t24-rem", "fwd", 2, 9, 20, [40], 16, 160, bias='a', res1='own', rem=True, layout='win', key=('tile', 1, 2, 4, 0, 8, 1), about=dict(ns=2, wb_persist=0, grid=8, ntiles=8)),
    T("t24-th12", "fwd", 11, 48, 128, [16], 16, 104, bias='o', res1='own', key=('tile', 1, 2, 4, 0, 12, 0), about=dict(ns=2, wb_persist=0, grid=352, ntiles=352)),
    T("t24-th12-rem", "fwd", 11, 48, 128, [8], 16, 72, bias='none', res1='own', rem=True, layout='chan', key=('tile', 1, 2, 4, 0, 12, 1), about=dict(ns=2, wb_persist=0, grid=352, ntiles=352)),
    T("t31", "fwd", 2, 20, 28, [32, 32], 24, 32, layout='win', key=('tile', 1, 3, 1, 0, 8, 0), about=dict(ns=2, wb_persist=0, grid=12, ntiles=12)),
    T("t31-rem", "fwd", 3, 12, 40, [32], 24, 32, bias='a', res1='own', rem=True, key=('tile', 1, 3, 1, 0, 8, 1), about=dict(ns=2, wb_persist=0, grid=18, ntiles=18)),
    T("t32", "fwd", 1, 17, 33, [32, 32], 24, 64, bias='o', res1='own', layout='chan', key=('tile', 1, 3, 2, 0, 8, 0), about=dict(ns=2, wb_persist=0, grid=9, ntiles=9)),
    T("t32-rem", "fwd", 2, 9, 20, [24, 4], 24, 64, bias='none', res1='own', rem=True, layout='win', key=('tile', 1, 3, 2, 0, 8, 1), about=dict(ns=2, wb_persist=0, grid=8, ntiles=8)),
    T("t34", "fwd", 2, 20, 28, [64, 4], 24, 104, key=('tile', 1, 3, 4, 0, 8, 0), about=dict(ns=3, wb_persist=0, grid=12, ntiles=12)),
    T("t34-rem", "fwd", 3, 12, 40, [96, 4, 96], 24, 104, bias='a', res1='own', rem=True, layout='chan', key=('tile', 1, 3, 4, 0, 8, 1), about=dict(ns=3, wb_persist=0, grid=18, ntiles=18)),
    T("t34-th12", "fwd", 11, 48, 128, [24, 4], 24, 72, bias='o', res1='own', layout='win', key=('tile', 1, 3, 4, 0, 12, 0), about=dict(ns=2, wb_persist=0, grid=352, ntiles=352)),
    T("t34-th12-rem", "fwd", 11, 48, 128, [8], 24, 72, bias='none', res1='own', rem=True, key=('tile', 1, 3, 4, 0, 12, 1), about=dict(ns=2, wb_persist=0, grid=352, ntiles=352)),
    T("t41", "fwd", 1, 17, 33, [64, 4], 32, 24, layout='chan', key=('tile', 1, 4, 1, 0, 8, 0), about=dict(ns=3, wb_persist=0, grid=9, ntiles=9)),
    T("t41-rem", "fwd", 2, 9, 20, [24, 4], 32, 24, bias='a', res1='own', rem=True, layout='win', key=('tile', 1, 4, 1, 0, 8, 1), about=dict(ns=2, wb_persist=0, grid=8, ntiles=8)),
    T("t42", "fwd", 2, 20, 28, [64, 4], 32, 40, bias='o', res1='own', key=('tile', 1, 4, 2, 0, 8, 0), about=dict(ns=3, wb_persist=0, grid=12, ntiles=12)),
    T("t42-rem", "fwd", 3, 12, 40, [40], 32, 40, bias='none', res1='own', rem=True, layout='chan', key=('tile', 1, 4, 2, 0, 8, 1), about=dict(ns=2, wb_persist=0, grid=18, ntiles=18)),
    T("t44", "fwd", 1, 17, 33, [128], 32, 72, layout='win', key=('tile', 1, 4, 4, 0, 8, 0), about=dict(ns=3, wb_persist=0, grid=9, ntiles=9)),
    T("t44-rem", "fwd", 2, 9, 20, [32], 32, 72, bias='a', res1='own', rem=True, key=('tile', 1, 4, 4, 0, 8, 1), about=dict(ns=2, wb_persist=0, grid=8, ntiles=8)),
    T("t11", "dgrad", 2, 20, 28, [24], 8, 64, res1='own', layout='chan', key=('tile', 0, 1, 1, 0, 8, 0), about=dict(ns=2, wb_persist=1, grid=12, ntiles=12)),
    T("t11-sm", "dgrad", 3, 12, 40, [24], 8, 32, layout='win', key=('tile', 0, 1, 1, 1, 8, 0), about=dict(ns=2, wb_persist=1, grid=18, ntiles=18)),
    T("t12", "dgrad", 1, 17, 33, [40], 8, 64, res1='own', key=('tile', 0, 1, 2, 0, 8, 0), about=dict(ns=2, wb_persist=1, grid=9, ntiles=9)),
    T("t12-sm", "dgrad", 2, 9, 20, [40], 8, 32, layout='chan', key=('tile', 0, 1, 2, 1, 8, 0), about=dict(ns=2, wb_persist=1, grid=8, ntiles=8)),
    T("t14", "dgrad", 2, 20, 28, [72], 8, 32, res1='own', layout='win', key=('tile', 0, 1, 4, 0, 8, 0), about=dict(ns=2, wb_persist=0, grid=12, ntiles=12)),
    T("t14-th12", "dgrad", 11, 48, 128, [72], 8, 8, key=('tile', 0, 1, 4, 0, 12, 0), about=dict(ns=2, wb_persist=0, grid=352, ntiles=352)),
    T("t21", "dgrad", 3, 12, 40, [32], 16, 40, res1='own', layout='chan', key=('tile', 0, 2, 1, 0, 8, 0), about=dict(ns=2, wb_persist=1, grid=18, ntiles=18)),
    T("t21-sm", "dgrad", 1, 17, 33, [32], 16, 24, layout='win', key=('tile', 0, 2, 1, 1, 8, 0), about=dict(ns=2, wb_persist=1, grid=9, ntiles=9)),
    T("t22", "dgrad", 2, 9, 20, [64], 16, 40, res1='own', key=('tile', 0, 2, 2, 0, 8, 0), about=dict(ns=2, wb_persist=1, grid=8, ntiles=8)),
    T("t22-sm", "dgrad", 2, 20, 28, [64], 16, 24, layout='chan', key=('tile', 0, 2, 2, 1, 8, 0), about=dict(ns=2, wb_persist=1, grid=12, ntiles=12)),
    T("t24", "dgrad", 3, 12, 40, [96, 4, 96], 16, 72, res1='own', layout='win', key=('tile', 0, 2, 4, 0, 8, 0), about=dict(ns=3, wb_persist=0, grid=18, ntiles=18)),
    T("t24-th12", "dgrad", 11, 48, 128, [96], 16, 16, key=('tile', 0, 2, 4, 0, 12, 0), about=dict(ns=2, wb_persist=0, grid=352, ntiles=352)),
    T("t31", "dgrad", 1, 17, 33, [32, 4], 24, 96, res1='own', layout='chan', key=('tile', 0, 3, 1, 0, 8, 0), about=dict(ns=3, wb_persist=0, grid=9, ntiles=9)),
    T("t32", "dgrad", 2, 9, 20, [64, 4, 32], 24, 96, layout='win', key=('tile', 0, 3, 2, 0, 8, 0), about=dict(ns=3, wb_persist=0, grid=8, ntiles=8)),
    T("t34", "dgrad", 2, 20, 28, [104], 24, 24, res1='own', key=('tile', 0, 3, 4, 0, 8, 0), about=dict(ns=2, wb_persist=0, grid=12, ntiles=12)),
    T("t34-th12", "dgrad", 11, 48, 128, [72], 24, 40, layout='chan', key=('tile', 0, 3, 4, 0, 12, 0), about=dict(ns=2, wb_persist=0, grid=352, ntiles=352)),
    T("t41", "dgrad", 3, 12, 40, [24, 8, 32], 32, 72, rg=[1, 0, 1], res1='own', layout='win', key=('tile', 0, 4, 1, 0, 8, 0), about=dict(ns=3, wb_persist=0, grid=18, ntiles=18)),
    T("t42", "dgrad", 1, 17, 33, [56], 32, 72, key=('tile', 0, 4, 2, 0, 8, 0), about=dict(ns=3, wb_persist=0, grid=9, ntiles=9)),
    T("t44", "dgrad", 2, 9, 20, [160], 32, 160, res1='own', layout='chan', key=('tile', 0, 4, 4, 0, 8, 0), about=dict(ns=3, wb_persist=0, grid=8, ntiles=8)),
    T("persist-sm-ragged-then-full", "fwd", 172, 20, 16, [32], 8, 32, res1='alias', key=('tile', 1, 1, 1, 1, 8, 0), about=dict(ns=2, wb_persist=1, grid=512, ntiles=516)),
    T("persist-anychunk-ragged-then-full", "fwd", 172, 20, 16, [40], 24, 64, bias='a', layout='chan', key=('tile', 1, 3, 2, 0, 8, 0), about=dict(ns=2, wb_persist=0, grid=512, ntiles=516)),
    T("persist-ragged-then-full", "dgrad", 172, 20, 16, [40], 16, 40, res1='own', key=('tile', 0, 2, 2, 0, 8, 0), about=dict(ns=2, wb_persist=1, grid=512, ntiles=516)),
    T("persist-nout2", "dgrad", 172, 20, 16, [32, 4, 32], 32, 32, key=('tile', 0, 4, 1, 0, 8, 0), about=dict(ns=2, wb_persist=0, grid=512, ntiles=516)),
    T("persist-th12", "fwd", 64, 48, 48, [8], 8, 72, bias='o', key=('tile', 1, 1, 4, 0, 12, 0), about=dict(ns=2, wb_persist=0, grid=512, ntiles=768)),
    T("cap78-ns3", "fwd", 6, 44, 120, [64, 4], 24, 104, res1='own', key=('tile', 1, 3, 4, 0, 8, 0), about=dict(ns=3, wb_persist=0, grid=288, ntiles=288)),
    T("cap78-ns3", "dgrad", 6, 44, 120, [72], 32, 72, key=('tile', 0, 4, 4, 0, 8, 0), about=dict(ns=3, wb_persist=0, grid=288, ntiles=288)),
    T("co224", "fwd", 1, 9, 20, [16], 8, 224, layout='chan', key=('tile', 1, 1, 4, 0, 8, 0), about=dict(ns=2, wb_persist=0, grid=4, ntiles=4)),
    T("rows-shape-without-a16", "fwd", 1, 16, 48, [32], 8, 32, res1='alias', key=('tile', 1, 1, 1, 1, 8, 0), about=dict(ns=2, wb_persist=1, grid=6, ntiles=6)),
    T("rows-shape-without-a16", "dgrad", 1, 16, 48, [32], 8, 32, key=('tile', 0, 1, 1, 1, 8, 0), about=dict(ns=2, wb_persist=1, grid=6, ntiles=6)),
    T("s-w14-short-last-strip", "fwd", 3, 5, 14, [64], 16, 64, res1='own', layout='win', bias='a', key=('small', 1), about=dict(s_rows=2, s_strips=3, s_nmb=1, grid=9)),
    T("s-w13", "fwd", 2, 9, 13, [24, 4, 40], 24, 40, layout='chan', bias='o', key=('small', 1), about=dict(s_rows=2, s_strips=5, s_nmb=1, grid=10)),
    T("s-w12-nmb2", "fwd", 2, 12, 12, [40, 4], 40, 48, res1='own', key=('small', 1), about=dict(s_rows=3, s_strips=4, s_nmb=2, grid=8)),
    T("s-w10", "fwd", 2, 11, 10, [32, 32], 32, 24, layout='win', bias='none', key=('small', 1), about=dict(s_rows=4, s_strips=3, s_nmb=1, grid=6)),
    T("s-w6-strip-per-image", "fwd", 4, 6, 6, [96], 48, 32, res1='own', layout='chan', key=('small', 1), about=dict(s_rows=6, s_strips=1, s_nmb=2, grid=4)),
    T("s-w5-nout2", "fwd", 2, 7, 5, [72, 8], 8, 56, key=('small', 1), about=dict(s_rows=7, s_strips=1, s_nmb=1, grid=2)),
    T("s-w4-b64", "fwd", 1, 4, 4, [24, 8, 32], 64, 104, rg=[1, 0, 1], res1='own', key=('small', 1), about=dict(s_rows=4, s_strips=1, s_nmb=2, grid=1)),
    T("s-co232", "fwd", 3, 8, 8, [16], 8, 232, layout='chan', key=('small', 1), about=dict(s_rows=6, s_strips=2, s_nmb=1, grid=6)),
    T("s-w14-short-last-strip", "dgrad", 3, 5, 14, [64], 16, 64, res1='own', layout='win', bias='a', key=('small', 0), about=dict(s_rows=2, s_strips=3, s_nmb=1, grid=9)),
    T("s-w13", "dgrad", 2, 9, 13, [24, 4, 40], 24, 40, layout='chan', bias='o', key=('small', 0), about=dict(s_rows=2, s_strips=5, s_nmb=1, grid=10)),
    T("s-w12-nmb2", "dgrad", 2, 12, 12, [40, 4], 40, 48, res1='own', key=('small', 0), about=dict(s_rows=3, s_strips=4, s_nmb=2, grid=8)),
    T("s-w10", "dgrad", 2, 11, 10, [32, 32], 32, 24, layout='win', bias='none', key=('small', 0), about=dict(s_rows=4, s_strips=3, s_nmb=1, grid=6)),
    T("s-w6-strip-per-image", "dgrad", 4, 6, 6, [96], 48, 32, res1='own', layout='chan', key=('small', 0), about=dict(s_rows=6, s_strips=1, s_nmb=2, grid=4)),
    T("s-w5-nout2", "dgrad", 2, 7, 5, [72, 8], 8, 56, key=('small', 0), about=dict(s_rows=7, s_strips=1, s_nmb=1, grid=2)),
    T("s-w4-b64", "dgrad", 1, 4, 4, [24, 8, 32], 64, 104, rg=[1, 0, 1], res1='own', key=('small', 0), about=dict(s_rows=4, s_strips=1, s_nmb=2, grid=1)),
    T("s-co232", "dgrad", 3, 8, 8, [16], 8, 232, layout='chan', key=('small', 0), about=dict(s_rows=6, s_strips=2, s_nmb=1, grid=6)),
    T("s-rem", "fwd", 2, 12, 12, [160], 40, 160, res1='own', rem=True, key=('small', 1), about=dict(s_rows=3, s_strips=4, s_nmb=2, grid=8)),
    T("s-rem-alias", "fwd", 4, 6, 6, [32], 16, 32, res1='alias', layout='win', key=('small', 1), about=dict(s_rows=6, s_strips=1, s_nmb=1, grid=4)),
    T("r32-8-None", "fwd", 1, 16, 48, [32], 8, 32, a16=True, bias='o', layout='win', key=('rows', 1, 1, 1, 0, 0), about=dict(r_rs=8, r_sx=2, r_sy=2, r_res_tile=0, grid=4)),
    T("r32-8-alias", "fwd", 1, 20, 70, [32], 8, 32, res1='alias', a16=True, bias='none', key=('rows', 1, 1, 1, 1, 0), about=dict(r_rs=8, r_sx=3, r_sy=3, r_res_tile=1, grid=9)),
    T("r32-8-own", "fwd", 1, 18, 50, [32], 8, 64, res1='own', a16=True, layout='chan', key=('rows', 1, 1, 1, 2, 0), about=dict(r_rs=8, r_sx=2, r_sy=3, r_res_tile=0, grid=6)),
    T("r32-8-down", "fwd", 1, 16, 48, [32], 8, 64, down=True, a16=True, bias='a', layout='win', key=('rows', 1, 1, 1, 0, 1), about=dict(r_rs=8, r_sx=2, r_sy=2, r_res_tile=0, grid=4)),
    T("r32-16-None", "fwd", 2, 17, 53, [32], 16, 32, a16=True, bias='o', key=('rows', 1, 1, 2, 0, 0), about=dict(r_rs=8, r_sx=2, r_sy=3, r_res_tile=0, grid=12)),
    T("r32-16-alias", "fwd", 1, 16, 48, [32], 16, 32, res1='alias', a16=True, bias='none', layout='chan', key=('rows', 1, 1, 2, 1, 0), about=dict(r_rs=8, r_sx=2, r_sy=2, r_res_tile=1, grid=4)),
    T("r32-16-own", "fwd", 1, 20, 70, [32], 16, 64, res1='own', a16=True, layout='win', key=('rows', 1, 1, 2, 2, 0), about=dict(r_rs=8, r_sx=3, r_sy=3, r_res_tile=0, grid=9)),
    T("r32-16-down", "fwd", 1, 20, 70, [32], 16, 64, down=True, a16=True, bias='a', key=('rows', 1, 1, 2, 0, 1), about=dict(r_rs=8, r_sx=3, r_sy=3, r_res_tile=0, grid=9)),
    T("r64-8-None", "fwd", 1, 18, 50, [64], 8, 64, a16=True, bias='o', layout='chan', key=('rows', 1, 2, 1, 0, 0), about=dict(r_rs=8, r_sx=2, r_sy=3, r_res_tile=0, grid=6)),
    T("r64-8-alias", "fwd", 2, 17, 53, [64], 8, 64, res1='alias', a16=True, bias='none', layout='win', key=('rows', 1, 2, 1, 1, 0), about=dict(r_rs=8, r_sx=2, r_sy=3, r_res_tile=1, grid=12)),
    T("r64-8-own", "fwd", 1, 16, 48, [64], 8, 32, res1='own', a16=True, key=('rows', 1, 2, 1, 2, 0), about=dict(r_rs=8, r_sx=2, r_sy=2, r_res_tile=0, grid=4)),
    T("r64-8-down", "fwd", 1, 18, 50, [64], 8, 32, down=True, a16=True, bias='a', layout='chan', key=('rows', 1, 2, 1, 0, 1), about=dict(r_rs=8, r_sx=2, r_sy=3, r_res_tile=0, grid=6)),
    T("r64-16-None", "fwd", 1, 20, 70, [64], 16, 64, a16=True, bias='o', layout='win', key=('rows', 1, 2, 2, 0, 0), about=dict(r_rs=8, r_sx=3, r_sy=3, r_res_tile=0, grid=9)),
    T("r64-16-alias", "fwd", 1, 18, 50, [64], 16, 64, res1='alias', a16=True, bias='none', key=('rows', 1, 2, 2, 1, 0), about=dict(r_rs=8, r_sx=2, r_sy=3, r_res_tile=1, grid=6)),
    T("r64-16-own", "fwd", 2, 17, 53, [64], 16, 32, res1='own', a16=True, layout='chan', key=('rows', 1, 2, 2, 2, 0), about=dict(r_rs=8, r_sx=2, r_sy=3, r_res_tile=0, grid=12)),
    T("r64-16-down", "fwd", 1, 16, 48, [64], 16, 32, down=True, a16=True, bias='a', layout='win', key=('rows', 1, 2, 2, 0, 1), about=dict(r_rs=8, r_sx=2, r_sy=2, r_res_tile=0, grid=4)),
    T("r32-8-None", "dgrad", 1, 16, 48, [32], 8, 32, a16=True, key=('rows', 0, 1, 1, 0, 0), about=dict(r_rs=8, r_sx=2, r_sy=2, r_res_tile=0, grid=4)),
    T("r32-8-None-down", "dgrad", 1, 20, 70, [64], 8, 32, down=True, a16=True, layout='chan', key=('rows', 0, 1, 1, 0, 1), about=dict(r_rs=8, r_sx=3, r_sy=3, r_res_tile=0, grid=9)),
    T("r32-8-own", "dgrad", 1, 20, 70, [64], 8, 32, res1='own', a16=True, layout='win', key=('rows', 0, 1, 1, 2, 0), about=dict(r_rs=8, r_sx=3, r_sy=3, r_res_tile=0, grid=9)),
    T("r32-8-own-down", "dgrad", 1, 18, 50, [64], 8, 32, res1='own', down=True, a16=True, key=('rows', 0, 1, 1, 2, 1), about=dict(r_rs=8, r_sx=2, r_sy=3, r_res_tile=0, grid=6)),
    T("r32-16-None", "dgrad", 1, 18, 50, [32], 16, 32, a16=True, layout='chan', key=('rows', 0, 1, 2, 0, 0), about=dict(r_rs=8, r_sx=2, r_sy=3, r_res_tile=0, grid=6)),
    T("r32-16-None-down", "dgrad", 1, 16, 48, [64], 16, 32, down=True, a16=True, layout='win', key=('rows', 0, 1, 2, 0, 1), about=dict(r_rs=8, r_sx=2, r_sy=2, r_res_tile=0, grid=4)),
    T("r32-16-own", "dgrad", 2, 17, 53, [64], 16, 32, res1='own', a16=True, key=('rows', 0, 1, 2, 2, 0), about=dict(r_rs=8, r_sx=2, r_sy=3, r_res_tile=0, grid=12)),
    T("r32-16-own-down", "dgrad", 1, 20, 70, [64], 16, 32, res1='own', down=True, a16=True, layout='chan', key=('rows', 0, 1, 2, 2, 1), about=dict(r_rs=8, r_sx=3, r_sy=3, r_res_tile=0, grid=9)),
    T("r64-8-None", "dgrad", 1, 16, 48, [64], 8, 64, a16=True, layout='win', key=('rows', 0, 2, 1, 0, 0), about=dict(r_rs=8, r_sx=2, r_sy=2, r_res_tile=0, grid=4)),
    T("r64-8-None-down", "dgrad", 1, 18, 50, [32], 8, 64, down=True, a16=True, key=('rows', 0, 2, 1, 0, 1), about=dict(r_rs=8, r_sx=2, r_sy=3, r_res_tile=0, grid=6)),
    T("r64-8-own", "dgrad", 1, 20, 70, [32], 8, 64, res1='own', a16=True, layout='chan', key=('rows', 0, 2, 1, 2, 0), about=dict(r_rs=8, r_sx=3, r_sy=3, r_res_tile=0, grid=9)),
    T("r64-8-own-down", "dgrad", 1, 16, 48, [32], 8, 64, res1='own', down=True, a16=True, layout='win', key=('rows', 0, 2, 1, 2, 1), about=dict(r_rs=8, r_sx=2, r_sy=2, r_res_tile=0, grid=4)),
    T("r64-16-None", "dgrad", 1, 18, 50, [64], 16, 64, a16=True, key=('rows', 0, 2, 2, 0, 0), about=dict(r_rs=8, r_sx=2, r_sy=3, r_res_tile=0, grid=6)),
    T("r64-16-None-down", "dgrad", 1, 20, 70, [32], 16, 64, down=True, a16=True, layout='chan', key=('rows', 0, 2, 2, 0, 1), about=dict(r_rs=8, r_sx=3, r_sy=3, r_res_tile=0, grid=9)),
    T("r64-16-own", "dgrad", 2, 17, 53, [32], 16, 64, res1='own', a16=True, layout='win', key=('rows', 0, 2, 2, 2, 0), about=dict(r_rs=8, r_sx=2, r_sy=3, r_res_tile=0, grid=12)),
    T("r64-16-own-down", "dgrad", 1, 18, 50, [32], 16, 64, res1='own', down=True, a16=True, key=('rows', 0, 2, 2, 2, 1), about=dict(r_rs=8, r_sx=2, r_sy=3, r_res_tile=0, grid=6)),
    T("r-one-strip", "fwd", 65, 16, 48, [32], 8, 32, res1='alias', a16=True, key=('rows', 1, 1, 1, 1, 0), about=dict(r_rs=16, r_sx=2, r_sy=1, r_res_tile=1, grid=130)),
    T("r-one-strip", "dgrad", 65, 16, 48, [32], 8, 32, a16=True, key=('rows', 0, 1, 1, 0, 0), about=dict(r_rs=16, r_sx=2, r_sy=1, r_res_tile=0, grid=130)),
]
