"""Shared by tests/test_pairing_fwd.py (no GPU) and tests/test_gpu_block3_fwd_pair.py: the shapes of the forward pair launch
(cgen_block3_pair with pre_act = 1), the argument records on given addresses, and the cases the entry points must decline.

A record describes one light Block forward: segments `seg_c` (a width that is no multiple of 8 is the parents: spatially constant,
zero-padded to 8) -> bottleneck `b` -> `co` output channels.  A is posterior-like ([h, pa, acts] -> 32), B prior-like ([z] or
[z, pa] -> 2 z_dim + width)."""
import ctypes as C
from collections import namedtuple

from causal_gen_amd import _lib

Rec = namedtuple("Rec", "seg_c b co")
Shape = namedtuple("Shape", "name n h w a b plan")  # plan: cgen_block3_pair_plan's out[0 .. 7], workgroups included

CTX = 4


def _ab(c, b, co_b, pa_in_b=True):
    return Rec([c, CTX, c], b, 32), Rec([c, CTX] if pa_in_b else [c], b, co_b)


# (bottleneck / 8, small, then per record: phase-B wave split, tile rows, workgroups -- the host planner's answers, asserted on the CPU)
SHAPES = [
    # tile instance, bottleneck 32: <4, 1, 8, 4, 8>; 2 x 2 x 3 = 12 tiles per record
    Shape("nb4-24x24", 2, 24, 24, *_ab(128, 32, 160), plan=(4, 0, 1, 8, 12, 4, 8, 12)),
    # partial tiles both ways: 20 rows = 2.5 tiles, 28 columns = 1.75
    Shape("nb4-20x28", 2, 20, 28, *_ab(128, 32, 160), plan=(4, 0, 1, 8, 12, 4, 8, 12)),
    # N odd: 3 x 2 x 3 = 18 + 18 workgroups
    Shape("nb4-3x24x24", 3, 24, 24, *_ab(128, 32, 160, pa_in_b=False), plan=(4, 0, 1, 8, 18, 4, 8, 18)),
    # bottleneck 24, the smallest N x H x W at which the planner gives the prior twelve-row tiles and the posterior eight: 516 tiles
    # of eight rows are two rounds over the 512 resident workgroups, 258 of twelve are one (3 x 12 x 1376: the fewest pixels over
    # every N <= 4, H <= 48 in steps of 4 and W a multiple of 16, found with cgen_block3_pair_plan; the plan is asserted in
    # test_pairing_fwd.py).  The posterior's grid is capped at the 512 resident workgroups: some walk two tiles
    Shape("nb3-th12-3x12x1376", 3, 12, 1376, *_ab(96, 24, 128), plan=(3, 0, 1, 8, 512, 4, 12, 258)),
    # ... and a small one where both get eight rows
    Shape("nb3-th8-3x20x28", 3, 20, 28, *_ab(96, 24, 128), plan=(3, 0, 1, 8, 18, 4, 8, 18)),
    # small-image instance: a workgroup per strip of 3 rows at 12 x 12, per image at 6 x 6
    Shape("small-3x12x12", 3, 12, 12, *_ab(160, 40, 192), plan=(5, 1, 0, 0, 12, 0, 0, 12)),
    Shape("small-3x6x6", 3, 6, 6, *_ab(192, 48, 224, pa_in_b=False), plan=(6, 1, 0, 0, 3, 0, 0, 3)),
]


def cp8(c):
    return -(-c // 8) * 8


def tensor_bytes(n, h, w, c):
    """Bytes of a dense NHWC binary16 tensor (channels padded to 8); the parents are [n][8]."""
    return n * cp8(c) * 2 if c % 8 else n * h * w * cp8(c) * 2


def view(ptr, n, h, w, c):
    cp = cp8(c)
    if c % 8:
        return _lib.View(ptr, cp, 0, 0, c, cp)
    return _lib.View(ptr, h * w * cp, w * cp, cp, c, 0)


FAKE = 1 << 20


def args(n, h, w, rec, ptr=None, pre_act=1):
    """cgen_block3_args of `rec` forward.  ptr: {"seg": [..], "mid", "out", "w_a", "bias_a", "w_b", "bias_b"} device addresses; None: an
    aligned stand-in for each (the planner is host code and dereferences nothing)."""
    p = ptr or {}
    a = _lib.Block3Args()
    a.dtype, a.n, a.h, a.w, a.nseg, a.nout, a.pre_act = _lib.F16, n, h, w, len(rec.seg_c), 1, pre_act
    for k, c in enumerate(rec.seg_c):
        a.seg[k] = view(p["seg"][k] if p else FAKE, n, h, w, c)
    a.w_a, a.bias_a = p.get("w_a", FAKE), p.get("bias_a", FAKE)
    a.mid, a.mid_aux = view(p.get("mid", FAKE), n, h, w, rec.b), _lib.NULL_VIEW
    o = a.o[0]
    o.w, o.bias = p.get("w_b", FAKE), p.get("bias_b", FAKE)
    o.out, o.aux, o.res1 = view(p.get("out", FAKE), n, h, w, rec.co), _lib.NULL_VIEW, _lib.NULL_VIEW
    return a


def plan(lib, a, b):
    out = (C.c_int32 * 8)()
    ok = lib.block3_pair_plan(C.byref(a), C.byref(b), out)
    return ok, tuple(out)


def declined(n, h, w, ra, rb, pa=None, pb=None):
    """(name, args a, args b) of every combination the forward pair must decline, derived from a served pair of records at n x h x w
    (a tile-instance shape with bottleneck 32; the addresses of the served pair, or stand-ins)."""
    A = lambda **kw: args(kw.pop("n", n), kw.pop("h", h), kw.pop("w", w), kw.pop("rec", ra), pa, **kw)
    B = lambda **kw: args(kw.pop("n", n), kw.pop("h", h), kw.pop("w", w), kw.pop("rec", rb), pb, **kw)
    out = []
    # one record pre_act and the other not
    b = B(pre_act=0)
    b.mid_aux = b.mid
    out.append(("pre_act-mixed", A(), b))
    a = A(pre_act=0)
    a.mid_aux = a.mid
    out.append(("pre_act-mixed-first", a, B()))
    # different image size or batch (smaller on the second record: it stays inside the buffers of the served pair)
    out.append(("height-differs", A(), B(h=h - 4)))
    out.append(("width-differs", A(), B(w=w - 4)))
    out.append(("batch-differs", A(), B(n=n - 1)))
    # different bottleneck (the second record's tensors are no larger)
    out.append(("bottleneck-differs", A(), B(rec=Rec(rb.seg_c, rb.b - 8, rb.co))))
    # a streaming instance: one 32-channel chunk in, bottleneck <= 16, one output pair (b3_plan: wb_persist)
    sm = Rec([32], 16, 32)
    out.append(("streaming", A(rec=sm), B(rec=Rec([32], 16, rb.co))))
    # remainder planes
    a = A()
    a.o[0].out_rem = 16 * tensor_bytes(n, h, w, ra.co)
    out.append(("remainder-plane-a", a, B()))
    b = B()
    b.o[0].out_rem = 16 * tensor_bytes(n, h, w, rb.co)
    out.append(("remainder-plane-b", A(), b))
    # a residual
    a = A()
    a.o[0].res1 = a.o[0].out
    out.append(("residual-a", a, B()))
    b = B()
    b.o[0].res1 = b.o[0].out
    out.append(("residual-b", A(), b))
    # combinations that are not instantiated: the records the other way round (A must be the one-pair instance), two narrow
    # outputs, a two-pair prior
    out.append(("swapped", B(), A()))
    out.append(("two-narrow", A(), B(rec=Rec(rb.seg_c, rb.b, 32))))
    out.append(("prior-two-pairs", A(), B(rec=Rec(rb.seg_c, rb.b, 64))))
    return out


def row_streaming(n=2, side=96):
    """A pair at 96 x 96 whose Blocks take the row-streaming instance where the row image of the weights is given (w_a16)."""
    a, b = args(n, side, side, Rec([64], 16, 64)), args(n, side, side, Rec([64], 16, 64))
    a.w_a16 = b.w_a16 = FAKE
    return a, b
