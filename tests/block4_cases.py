"""The case table of the fused default Block (cgen_block4, csrc/block4.hip), shared by tests/test_block4_cases.py (no GPU) and
tests/test_gpu_block4_f64.py: shapes, layouts, the argument record on given addresses, a plain-Python mirror of b4_fill and of the
launch decision, the instance key cgen_block4_plan must name for each case, and the records the entry points decline.

A case describes the FORWARD Block  cat(segs) -> b -> b -> b -> co  and a direction:
  fwd    seg = the segments, mid[0..2] = t0, t1, t2 (b channels), one output of co channels (+ biases, res1, remainder planes);
  dgrad  seg[0] = grad_out (co channels), mid[0..2] = the gradients w.r.t. t2, t1, t0, mid_aux[0..2] = t2, t1, t0, one output per
         differentiable segment k (`rg`): out.c = segs[k], aux = the forward segment, res1 = the gradient accumulated so far where
         `res[j]` says so.
Channel counts that are no multiple of 8 are zero padded to 8 through cgen_view.cpad: the bottleneck tensors (b = 4, 5, 6, 12, 20, 36,
60), a 12-channel segment (strided like every other tensor), and the 6-channel parents, which are spatially constant (strides 0, as
engine.from_parents makes them).  Neither ragged segment wants a gradient.

Instance keys, from cgen_block4_plan's out[0 .. 2]:
  ("fwd", NB8, NW)     blk4_kernel<true, NB8, NW>     NW = 8 up to 1024 tiles, 4 above
  ("dgrad", NB8, 4)    blk4_kernel<false, NB8, 4>
  ("pair", NB8)        blk4_pair_kernel<NB8>          (cgen_block4_pair_plan)
NB8 = ceil(b / 8) in {1, 2, 3, 4, 5, 6, 8}: 49 .. 56 channels have no instance, 57 .. 64 run as 8.

Layouts (`layout`), as in tests/block_cases.py: "dense" the parent is the view (channels rounded up to 8); "chan" a channel slice of a
parent 16 channels wider, from channel 8; "win" a window of a parent with one more image, two more rows, three more columns and 8 more
channels.  Everything of a parent that is not the view or its cpad zeros is NaN (tests/gpu_views.Arena.place)."""
import ctypes as C

from block_cases import cp8, parent_shape
from causal_gen_amd import _lib

PLAN_INTS = 16
PLAN_FIELDS = {"ntiles": 3, "grid": 4, "lds": 5, "xcd_order": 6, "tiles_x": 7, "tiles_y": 8, "nch0": 9}
FAKE = 1 << 20
TH, TW = 8, 16
NB8S = (1, 2, 3, 4, 5, 6, 8)


class Case:
    dt = "h16"

    def __init__(self, name, dir, n, h, w, segs, b, co, rg=None, bias="1111", res=None, rem="", layout="dense", key=None):
        self.name, self.dir, self.n, self.h, self.w = name, dir, n, h, w
        self.segs, self.b, self.co = list(segs), b, co
        self.rg = list(rg) if rg is not None else [int(c % 8 == 0) for c in segs]
        self.bias = bias      # forward: which of bias[0], bias[1], bias[2], o[0].bias are given ("1" / "0")
        self.rem = rem        # forward: "" or any of "o" (out_rem) and "r" (res1_rem)
        self.layout = layout
        self.key = key
        if dir == "fwd":
            self.res = [bool(res)] if not isinstance(res, (list, tuple)) else list(res)  # o[0].res1 given
        else:
            self.res = list(res) if res is not None else [0] * len(self.dsegs)            # per output: accumulates
        assert dir in ("fwd", "dgrad") and layout in ("dense", "chan", "win") and len(bias) == 4
        assert all(not r or c % 8 == 0 for c, r in zip(self.segs, self.rg)) and len(self.res) == self.nout
        assert "r" not in rem or self.res[0]

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
    def nb8(self):
        return {7: 8}.get(-(-self.b // 8), -(-self.b // 8))

    @property
    def tiles(self):
        return -(-self.w // TW), -(-self.h // TH)

    @property
    def ntiles(self):
        return self.n * self.tiles[0] * self.tiles[1]

    @property
    def nch0(self):
        return sum(-(-c // 32) for c in (self.segs if self.dir == "fwd" else [self.co]))

    def seg_off(self, k):
        return sum(self.segs[:k])

    def flat(self, c):
        """A spatially constant segment (strides 0): the parents."""
        return c % 8 != 0 and c != 12


def view_of(case, ptr, shape, flat=False):
    """The cgen_view of a tensor of `shape` whose first element is at `ptr`, in the case's layout (flat: the parents segment)."""
    n, h, w, c = shape
    if flat:
        return _lib.View(ptr, cp8(c), 0, 0, c, cp8(c))
    (pn, ph, pw, pc), _ = parent_shape(case, shape)
    return _lib.View(ptr, ph * pw * pc, pw * pc, pc, c, cp8(c) if c % 8 else 0)


def args(case, ptr=None):
    """cgen_block4_args of the case.  ptr: role -> device address ("s0" .., "w0" .. "w2", "bias0" .. "bias2", "mid0" .., "aux0" ..,
    "wo0" .., "biaso", "out0" .., "oaux0" .., "res0" .., and "rem_out" / "rem_res": byte offsets of the remainder planes); None:
    aligned stand-ins (cgen_block4_supported and cgen_block4_plan are host code and dereference nothing)."""
    P = (lambda k, d=FAKE: ptr[k]) if ptr is not None else (lambda k, d=FAKE: d)
    n, h, w, b = case.n, case.h, case.w, case.b
    a = _lib.Block4Args()
    fwd = case.dir == "fwd"
    a.dtype, a.n, a.h, a.w, a.nout, a.fwd, a.b = _lib.F16, n, h, w, case.nout, int(fwd), b
    for k in range(3):
        a.wimg[k] = P(f"w{k}")
        a.mid[k] = view_of(case, P(f"mid{k}"), (n, h, w, b))
        a.mid_aux[k] = _lib.NULL_VIEW if fwd else view_of(case, P(f"aux{k}"), (n, h, w, b))
        a.bias[k] = P(f"bias{k}") if fwd and case.bias[k] == "1" else None
    if fwd:
        a.nseg = len(case.segs)
        for k, c in enumerate(case.segs):
            a.seg[k] = view_of(case, P(f"s{k}"), (n, h, w, c), case.flat(c))
        o = a.o[0]
        o.w, o.bias = P("wo0"), (P("biaso") if case.bias[3] == "1" else None)
        o.out, o.aux = view_of(case, P("out0"), (n, h, w, case.co)), _lib.NULL_VIEW
        o.res1 = view_of(case, P("res0"), (n, h, w, case.co)) if case.res[0] else _lib.NULL_VIEW
        o.out_rem = P("rem_out", 1 << 24) if "o" in case.rem else 0
        o.res1_rem = P("rem_res", 1 << 24) if "r" in case.rem else 0
    else:
        a.nseg = 1
        a.seg[0] = view_of(case, P("s0"), (n, h, w, case.co))
        for j, k in enumerate(case.dsegs):
            o = a.o[j]
            shape = (n, h, w, case.segs[k])
            o.w, o.bias = P(f"wo{j}"), None
            o.out, o.aux = view_of(case, P(f"out{j}"), shape), view_of(case, P(f"oaux{j}"), shape)
            o.res1 = view_of(case, P(f"res{j}"), shape) if case.res[j] else _lib.NULL_VIEW
    return a


def key_of(out):
    return ("fwd" if out[0] else "dgrad", out[1], out[2])


def plan(lib, a):
    """(what cgen_block4_plan answers, instance key or None, plan values by name)."""
    out = (C.c_int32 * PLAN_INTS)()
    ok = lib.block4_plan(C.byref(a), out)
    if not ok:
        return 0, None, {}
    assert not any(out[10:])
    return ok, key_of(tuple(out)), {k: out[i] for k, i in PLAN_FIELDS.items()}


# ------------------------------------------------------------------------------------------------- the mirror of b4_fill / b4_plan
def _view_ok(v, n, h, w):
    if not v.p:
        return True
    ext = (n * v.sn + (h + TH + 4) * v.sh + (w + TW + 4) * v.sw + v.c + 64) * 2
    if ext >= 1 << 31 or v.sn < 0 or v.sh < 0 or v.sw < 0:
        return False
    return not (v.p % 16 or (v.sn * 2) % 16 or (v.sh * 2) % 16 or (v.sw * 2) % 16)


def _groups_ok(v):
    return v.c % 8 == 0 or v.cpad >= cp8(v.c)


def lds_bytes(nb8):
    ps = (2 * ((nb8 + 1) // 2) + 1) * 16
    return (240 + 180 + 128) * ps + (3 * 64 * 4 + 256 * 4) + 385 * 16


def mirror(a):
    """What cgen_block4_plan must answer for the record `a`, from a reading of b4_fill and b4_plan at the default knobs: None where
    the record is declined, else (key, plan values)."""
    if a.dtype != _lib.F16 or not 1 <= a.nseg <= 3 or a.n <= 0 or a.h < 1 or a.w < 1:
        return None
    if not 1 <= a.nout <= 3 or not 1 <= a.b <= 64:
        return None
    fwd = a.fwd != 0
    if fwd and a.nout != 1:
        return None
    nb8 = (a.b + 7) // 8
    if nb8 == 7:
        return None
    nch = 0
    for s in range(a.nseg):
        v = a.seg[s]
        if not v.p or v.c <= 0 or not _groups_ok(v) or not _view_ok(v, a.n, a.h, a.w):
            return None
        nch += (v.c + 31) // 32
    for k in range(3):
        m, x = a.mid[k], a.mid_aux[k]
        if not a.wimg[k] or not m.p or m.c != a.b or not _groups_ok(m) or not _view_ok(m, a.n, a.h, a.w):
            return None
        if fwd:
            if x.p:
                return None
        elif not x.p or x.c != a.b or not _groups_ok(x) or not _view_ok(x, a.n, a.h, a.w):
            return None
    for j in range(a.nout):
        s = a.o[j]
        if not s.w or not s.out.p or s.out.c <= 0 or s.out.c % 8 or (fwd and s.out.c > 256) or not _view_ok(s.out, a.n, a.h, a.w):
            return None
        if fwd:
            if s.aux.p:
                return None
        elif not s.aux.p or s.aux.c != s.out.c or not _view_ok(s.aux, a.n, a.h, a.w):
            return None
        if s.res1.p and (s.res1.c != s.out.c or not _view_ok(s.res1, a.n, a.h, a.w)):
            return None
        if not (0 <= s.out_rem < 1 << 30 and 0 <= s.res1_rem < 1 << 30) or (not fwd and (s.out_rem or s.res1_rem)):
            return None
    tx, ty = -(-a.w // TW), -(-a.h // TH)
    nt = a.n * tx * ty
    if nt >= 1 << 30:
        return None
    nw = 8 if fwd and nt <= 1024 else 4
    return ("fwd" if fwd else "dgrad", nb8, nw), dict(ntiles=nt, grid=nt, lds=lds_bytes(nb8), xcd_order=int(nt >= 512), tiles_x=tx, tiles_y=ty,
                                                     nch0=nch)


# ------------------------------------------------------------------------------------------------- what the entry points decline
def _set(path, value):
    def f(a):
        obj, names = a, path.split(".")
        for nm in names[:-1]:
            obj = getattr(obj, nm[:-3])[int(nm[-2])] if nm.endswith("]") else getattr(obj, nm)
        setattr(obj, names[-1], value)
    return f


def _bump(path, by):
    def f(a):
        obj, names = a, path.split(".")
        for nm in names[:-1]:
            obj = getattr(obj, nm[:-3])[int(nm[-2])] if nm.endswith("]") else getattr(obj, nm)
        setattr(obj, names[-1], getattr(obj, names[-1]) + by)
    return f


def _all_b(b):
    def f(a):
        a.b = b
        for k in range(3):
            a.mid[k].c, a.mid[k].cpad = b, cp8(b)
            if not a.fwd:
                a.mid_aux[k].c, a.mid_aux[k].cpad = b, cp8(b)
    return f


def _two_out(a):
    a.nout = 2
    a.o[1] = a.o[0]


def _co(c):
    def f(a):
        a.o[0].out.c = c
        if a.o[0].res1.p:
            a.o[0].res1.c = c
    return f


def _fwd_aux(a):
    a.mid_aux[1] = a.mid[1]


def _no_wimg(a):
    a.wimg[2] = None


def _huge(a):  # 2^31 bytes: ((n - 1) sn + ...) * 2 -- by address arithmetic only, nothing of it exists
    a.seg[0].sn = (1 << 30) // a.n + 8


_FWD = Case("base", "fwd", 2, 9, 17, [40, 12], 16, 24, res=True, rem="or")
_DG = Case("base", "dgrad", 2, 9, 17, [40, 16], 16, 24, res=[1, 0])
# (name, base case, change of its argument record; "gpu": also launched through cgen_block4 on real tensors, which must raise and write nothing)
DECLINED = (
    [(f"b{b}", _FWD, _all_b(b), True) for b in (0, 49, 50, 51, 52, 53, 54, 55, 56, 65)]
    + [(f"dgrad-b{b}", _DG, _all_b(b), True) for b in (0, 49, 56, 65)]
    + [
        ("nseg0", _FWD, _set("nseg", 0), True),
        ("nseg4", _FWD, _set("nseg", 4), True),
        ("fwd-two-outputs", _FWD, _two_out, True),
        ("fwd-co264", _FWD, _co(264), True),
        ("out-c-not-a-multiple-of-8", _FWD, _co(20), True),
        ("dgrad-out-c-not-a-multiple-of-8", _DG, _set("o[1].out.c", 12), True),
        ("misaligned-pointer", _FWD, _bump("seg[0].p", 8), True),
        ("misaligned-mid-pointer", _DG, _bump("mid[2].p", 2), True),
        ("misaligned-stride", _FWD, _bump("o[0].out.sh", 4), True),
        ("negative-stride", _FWD, _set("seg[0].sh", -16), True),
        ("mid-c-not-b", _FWD, _set("mid[1].c", 8), True),
        ("fwd-with-mid-aux", _FWD, _fwd_aux, True),
        ("dgrad-without-mid-aux", _DG, _set("mid_aux[1].p", None), True),
        ("dgrad-without-out-aux", _DG, _set("o[0].aux.p", None), True),
        ("dgrad-with-out-rem", _DG, _set("o[0].out_rem", 4096), True),
        ("dgrad-with-res1-rem", _DG, _set("o[0].res1_rem", 4096), True),
        ("ragged-segment-without-cpad", _FWD, _set("seg[1].cpad", 0), True),
        ("ragged-mid-without-cpad", Case("base20", "fwd", 2, 9, 17, [40], 20, 24), _set("mid[0].cpad", 0), True),
        ("f32", _FWD, _set("dtype", _lib.F32), True),
        ("negative-out-rem", _FWD, _set("o[0].out_rem", -16), True),
        ("view-of-2^31-bytes", _FWD, _huge, False),   # host only: stand-in addresses
        ("null-weight-image", _FWD, _no_wimg, True),
    ]
)


# ------------------------------------------------------------------------------------------------- the reachability sweep
def sweep_records():
    """Argument records over every axis at which b4_fill / b4_plan branch: b 1 .. 64 and beyond, 1-3 segments of every width class,
    1-3 outputs, tile counts around 512 and 1024, both directions, remainder planes -- then every declined change on top of two bases."""
    shapes = [(1, 1, 1), (2, 4, 4), (2, 8, 16), (2, 9, 17), (3, 7, 9), (1, 13, 33), (32, 28, 28), (86, 17, 17), (64, 17, 17), (171, 17, 17),
              (128, 32, 17), (1024, 1, 1), (1025, 1, 1), (511, 2, 3), (512, 8, 16)]
    seg_sets = [[8], [16], [32], [40], [128], [40, 12], [32, 6, 16], [24, 6], [96, 6, 96], [264]]
    recs = []
    for n, h, w in shapes:
        for segs in seg_sets:
            for b in list(range(1, 67, 3)) + [8, 16, 24, 32, 48, 56, 57, 64]:
                for co in (8, 24, 160, 256, 264):
                    recs.append(args(Case("sweep", "fwd", n, h, w, segs, b, co, res=co == 24, rem="or" if co == 24 else "")))
                    if all(c % 8 == 0 or len(segs) > 1 for c in segs):
                        rg = [int(c % 8 == 0) for c in segs]
                        recs.append(args(Case("sweep", "dgrad", n, h, w, segs, b, co, rg=rg, res=[k % 2 for k in range(sum(rg))])))
    for _, base, change, _ in DECLINED:
        a = args(base)
        change(a)
        recs.append(a)
    return recs


def T(*a, **k):
    return Case(*a, **k)


# One case (at least) per instance key, then the conditions the kernel branches on.  Names say what a case is about.  Shapes are the
# smallest that reach the condition: 1 x 1 and 4 x 4 (a tile mostly outside the image), 8 x 16 (exactly one tile), 9 x 17 (a last tile
# of one row and one column: tiles_x = 2 with a 1-pixel last tile, the second inv[][] column), 7 x 9 and 13 x 33 (ragged; 13 x 33:
# tiles_x = 3), 86 x 17 x 17 = 516 tiles (eight waves, the XCD order's identity tail of 4), and for the four-wave forward kernel more
# than 1024 tiles with ntiles % 8 != 0: 171 x 17 x 17 = 1026, 257 x 9 x 17 = 1028, 1027 x 2 x 3 and 1030 x 1 x 2 (one tile per image).
# Input widths: 8 (lane half kg = 1 reads zeros), 16 (one step), 32, 40 (ragged second chunk), 12 (cpad), 6 (parents); phase-0 chunk
# counts 1, 2, 3, 4, 6 (the two-stage pipeline's head and tail).
CASES = [
    T("b4-1x1", "fwd", 3, 1, 1, [8], 4, 8, key=("fwd", 1, 8)),
    T("b5-4x4-res", "fwd", 2, 4, 4, [16], 5, 24, res=True, layout="chan", key=("fwd", 1, 8)),
    T("b6-9x17-parents", "fwd", 2, 9, 17, [8, 6], 6, 8, bias="1010", layout="win", key=("fwd", 1, 8)),
    T("b8-8x16-some-biases", "fwd", 2, 8, 16, [32], 8, 40, bias="0101", layout="win", key=("fwd", 1, 8)),
    T("b12-9x17-both-rem", "fwd", 2, 9, 17, [40], 12, 24, res=True, rem="or", key=("fwd", 2, 8)),
    T("b16-13x33-chunks4", "fwd", 1, 13, 33, [128], 16, 40, bias="0000", layout="chan", key=("fwd", 2, 8)),
    T("b20-7x9-out-rem", "fwd", 3, 7, 9, [32, 6, 16], 20, 40, rem="o", layout="win", key=("fwd", 3, 8)),
    T("b24-13x33-co256-res-rem", "fwd", 1, 13, 33, [40, 12], 24, 256, res=True, rem="r", key=("fwd", 3, 8)),
    T("b32-9x17-chunks3", "fwd", 2, 9, 17, [96], 32, 8, res=True, layout="chan", key=("fwd", 4, 8)),
    T("b36-8x16-chunks6", "fwd", 2, 8, 16, [96, 6, 40], 36, 24, bias="1101", key=("fwd", 5, 8)),
    T("b40-7x9-res", "fwd", 3, 7, 9, [32, 6, 40], 40, 40, res=True, layout="win", key=("fwd", 5, 8)),
    T("b48-4x4-co256", "fwd", 2, 4, 4, [16, 8], 48, 256, layout="chan", key=("fwd", 6, 8)),
    T("b60-9x17", "fwd", 2, 9, 17, [8], 60, 24, res=True, rem="or", layout="win", key=("fwd", 8, 8)),
    T("b64-13x33-three-segments", "fwd", 1, 13, 33, [40, 12, 32], 64, 40, res=True, key=("fwd", 8, 8)),
    T("tiles516-eight-waves-xcd-tail", "fwd", 86, 17, 17, [16], 8, 8, res=True, key=("fwd", 1, 8)),
    T("tiles1026-b4", "fwd", 171, 17, 17, [8], 4, 8, key=("fwd", 1, 4)),
    T("tiles1028-b12", "fwd", 257, 9, 17, [16], 12, 16, res=True, layout="win", key=("fwd", 2, 4)),
    T("tiles1026-b20", "fwd", 171, 17, 17, [8, 6], 20, 8, bias="0110", key=("fwd", 3, 4)),
    T("tiles1028-b32", "fwd", 257, 9, 17, [16], 32, 8, layout="chan", key=("fwd", 4, 4)),
    T("tiles1027-b36", "fwd", 1027, 2, 3, [8], 36, 16, res=True, rem="or", key=("fwd", 5, 4)),
    T("tiles1027-b48", "fwd", 1027, 2, 3, [16], 48, 8, key=("fwd", 6, 4)),
    T("tiles1030-b64", "fwd", 1030, 1, 2, [8], 64, 16, res=True, key=("fwd", 8, 4)),
    T("b4-9x17-g8", "dgrad", 2, 9, 17, [8], 4, 8, key=("dgrad", 1, 4)),
    T("b8-7x9-two-outputs", "dgrad", 3, 7, 9, [16, 6, 24], 8, 24, res=[1, 0], layout="win", key=("dgrad", 1, 4)),
    T("b12-13x33-out264-g160", "dgrad", 1, 13, 33, [264], 12, 160, res=[1], key=("dgrad", 2, 4)),
    T("b16-8x16", "dgrad", 2, 8, 16, [32], 16, 40, layout="chan", key=("dgrad", 2, 4)),
    T("b20-4x4-three-outputs-g224", "dgrad", 2, 4, 4, [8, 16, 40], 20, 224, res=[0, 1, 1], layout="chan", key=("dgrad", 3, 4)),
    T("b24-8x16", "dgrad", 2, 8, 16, [32], 24, 8, res=[1], layout="win", key=("dgrad", 3, 4)),
    T("b32-9x17-ragged-parents", "dgrad", 2, 9, 17, [40, 12], 32, 24, res=[1], key=("dgrad", 4, 4)),
    T("b36-1x1", "dgrad", 3, 1, 1, [16, 8], 36, 40, res=[1, 0], key=("dgrad", 5, 4)),
    T("b40-7x9", "dgrad", 3, 7, 9, [40, 6, 32], 40, 24, res=[0, 1], layout="win", key=("dgrad", 5, 4)),
    T("b48-13x33-g160", "dgrad", 1, 13, 33, [24], 48, 160, layout="chan", key=("dgrad", 6, 4)),
    T("b60-9x17-two-outputs", "dgrad", 2, 9, 17, [32, 32], 60, 24, res=[0, 1], key=("dgrad", 8, 4)),
    T("b64-4x4", "dgrad", 2, 4, 4, [96], 64, 8, res=[1], layout="win", key=("dgrad", 8, 4)),
    T("tiles516-xcd-tail", "dgrad", 86, 17, 17, [8], 8, 16, res=[1], key=("dgrad", 1, 4)),
    T("tiles1026", "dgrad", 171, 17, 17, [16], 16, 8, key=("dgrad", 2, 4)),
]

# cgen_block4_pair: two data-gradient problems of one bottleneck class and different shape -- 8 tiles (2 x 9 x 17) beside 7 (7 x 5 x 9)
PAIRS = []
for _nb8, (_ba, _bb) in zip(NB8S, ((4, 8), (12, 16), (20, 24), (32, 28), (40, 36), (48, 44), (60, 64))):
    PAIRS.append((T(f"pairA-b{_ba}", "dgrad", 2, 9, 17, [40, 6, 16], _ba, 24, res=[1, 0], layout="win", key=("pair", _nb8)),
                  T(f"pairB-b{_bb}", "dgrad", 7, 5, 9, [32], _bb, 40, layout="chan", key=("pair", _nb8))))

EXPECTED_KEYS = ({("fwd", nb8, nw) for nb8 in NB8S for nw in (4, 8)} | {("dgrad", nb8, 4) for nb8 in NB8S})
