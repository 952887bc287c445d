"""Case table of the element-wise NHWC kernels (csrc/elementwise.hip), shared by tests/test_gpu_elementwise.py (runs each case
against an f64 reference) and tests/test_elementwise_cases.py (checks, without a GPU, that the table reaches every launch arm).

Every NHWC view of a case lies in a parent tensor [n + pad, h + pad, w + pad, off + c + cext] at channel offset `off`; the parent is
allocated whole (its base is at least 256-byte aligned), so the byte alignment of a view is `off * esz` and its strides are the
parent's.  `arm()` mirrors the host-side choice of the kernel instance (vec4_ok and the axpby flat predicate of elementwise.hip)."""
from dataclasses import dataclass, field

GRID_CAP = 4096 * 256  # grid_for: at most 4096 blocks of 256 threads; more work items wrap round the grid-stride loop
BATCH_REDUCE_CAP = 4096 * 64  # batch_reduce_kernel: a block owns 64 per-sample elements per pass
NO_SPLIT = 1 << 30  # axpby c_from that scales no channel by beta

# entry points whose instance is chosen per call by vec4_ok (DISPATCH_TV): 4-channel vector body or scalar body
TV_OPS = ("avgpool_fwd", "avgpool_bwd", "adaptive_avgpool_fwd", "adaptive_avgpool_bwd", "upsample_fwd", "upsample_bwd",
          "batch_broadcast", "axpby")
# one instance per dtype
PLAIN_OPS = ("batch_reduce", "nchw_to_nhwc", "nhwc_to_nchw", "im2col_strided", "col2im_strided", "unary_fwd", "unary_bwd")
ACC_OPS = ("avgpool_bwd", "adaptive_avgpool_bwd", "upsample_bwd", "axpby", "batch_reduce", "col2im_strided", "unary_bwd")
ALL_ARMS = {op: ({"vec", "scalar", "flat"} if op == "axpby" else {"vec", "scalar"}) if op in TV_OPS else {"plain"}
            for op in TV_OPS + PLAIN_OPS}
UNARY = ("relu", "gelu", "leaky_relu", "clamp_min", "add")
DTYPES = ("f32", "h16")


@dataclass(frozen=True)
class Case:
    op: str
    dt: str  # "f32" or "h16" (the library's 16-bit format, cgen_h16_format())
    n: int
    h: int  # spatial size of the op's OUTPUT (forward ops) / of the gradient it writes (backward ops)
    w: int
    c: int
    off: int = 0  # channel offset of every NHWC view in its parent
    cext: int = 0  # parent channels after the view
    pad: int = 0  # parent rows / columns / samples beyond the view
    acc: int = 0
    p: tuple = field(default_factory=tuple)  # op parameters, see views()
    flat_axpy: bool = False  # axpby through Engine.flat_axpy's two calls (whole rows of 1024 + a tail) on `count` = n*h*w*c floats

    @property
    def esz(self):
        return 4 if self.dt == "f32" else 2

    @property
    def cpar(self):
        return self.off + self.c + self.cext

    def id(self):
        s = f"{self.op}-{self.dt}-{arm(self)}-n{self.n}x{self.h}x{self.w}x{self.c}"
        if self.off or self.cext:
            s += f"-off{self.off}of{self.cpar}"
        if self.pad:
            s += f"-pad{self.pad}"
        if self.op in ACC_OPS:
            s += f"-acc{self.acc}"
        if self.p:
            s += "-" + "-".join(str(x) for x in self.p)
        if self.flat_axpy:
            s += "-flat_axpy"
        return s


def views(case):
    """role -> (n, h, w, c) of every NHWC view the entry point reads or writes ('out' is the one it writes)."""
    n, h, w, c = case.n, case.h, case.w, case.c
    op = case.op
    if op == "avgpool_fwd":
        d, = case.p
        return {"in": (n, h * d, w * d, c), "out": (n, h, w, c)}
    if op == "avgpool_bwd":  # (h, w): the input gradient; gout is [h / d, w / d]
        d, = case.p
        return {"gout": (n, h // d, w // d, c), "out": (n, h, w, c)}
    if op == "adaptive_avgpool_fwd":
        hi, wi = case.p
        return {"in": (n, hi, wi, c), "out": (n, h, w, c)}
    if op == "adaptive_avgpool_bwd":
        ho, wo = case.p
        return {"gout": (n, ho, wo, c), "out": (n, h, w, c)}
    if op == "upsample_fwd":
        hi, wi, _bias = case.p
        return {"in": (n, hi, wi, c), "out": (n, h, w, c)}
    if op == "upsample_bwd":
        ho, wo = case.p
        return {"gout": (n, ho, wo, c), "out": (n, h, w, c)}
    if op == "batch_broadcast":
        return {"out": (n, h, w, c)}
    if op == "axpby":
        _alpha, _beta, _c_from, fill = case.p
        return {"out": (n, h, w, c)} if fill else {"in": (n, h, w, c), "out": (n, h, w, c)}
    if op == "batch_reduce":
        return {"in": (n, h, w, c)}
    if op == "nchw_to_nhwc":
        return {"out": (n, h, w, c)}
    if op == "nhwc_to_nchw":
        return {"in": (n, h, w, c)}
    if op == "im2col_strided":  # (h, w, c): the input image; out has the conv's output size and c * ks^2 (+ cpad) channels
        ks, st, pd, _cpad = case.p
        ho, wo = (h + 2 * pd - ks) // st + 1, (w + 2 * pd - ks) // st + 1
        return {"in": (n, h, w, c), "out": (n, ho, wo, c * ks * ks)}
    if op == "col2im_strided":
        ks, st, pd = case.p
        ho, wo = (h + 2 * pd - ks) // st + 1, (w + 2 * pd - ks) // st + 1
        return {"gcol": (n, ho, wo, c * ks * ks), "out": (n, h, w, c)}
    if op == "unary_fwd":
        return {"in": (n, h, w, c), "out": (n, h, w, c)}
    if op == "unary_bwd":
        return {"x": (n, h, w, c), "gout": (n, h, w, c), "out": (n, h, w, c)}
    raise KeyError(op)


def parent_shape(case, shape):
    """Shape of the parent tensor of a view of `shape` (views whose channel count differs from case.c -- the im2col column
    tensor -- live alone in a parent of their own)."""
    n, h, w, c = shape
    if c != case.c:  # (im2col: the kernel writes the zero channels up to out.cpad too; two spare channels after them)
        cp = max(c, case.p[3]) + 2 if case.op == "im2col_strided" else c
        return (n + case.pad, h + case.pad, w + case.pad, cp), 0
    return (n + case.pad, h + case.pad, w + case.pad, case.cpar), case.off


def view_layout(case, shape):
    """(byte offset from the parent base, sn, sh, sw) in elements, as torch slicing of the parent gives them."""
    (_, hp, wp, cp), off = parent_shape(case, shape)
    return off * case.esz, hp * wp * cp, wp * cp, cp


def vec4_ok(esz, c, layouts):
    """elementwise.hip vec4_ok: channels a multiple of 4, base and every stride a multiple of 4 elements' bytes."""
    if c % 4:
        return False
    q = 4 * esz
    return all(p % q == 0 and (sn * esz) % q == 0 and (sh * esz) % q == 0 and (sw * esz) % q == 0 for p, sn, sh, sw in layouts)


def axpby_flat(esz, n, h, w, c, c_from, layouts):
    """cgen_axpby's flat predicate: whole contiguous tensors, 16-byte aligned, no per-channel scaling."""
    def flat(lay):
        p, sn, sh, sw = lay
        return sw == c and sh == w * c and sn == h * w * c and p % 16 == 0
    return c % (16 // esz) == 0 and c_from >= c and all(flat(x) for x in layouts)


def flat_axpy_calls(count):
    """The axpby calls Engine.flat_axpy makes for `count` contiguous f32: (n, h, w, c, byte offset) -- rows of 1024, then a tail."""
    cols, rows = 1024, count // 1024
    calls = []
    if rows:
        calls.append((1, 1, rows, cols, 0))
    if count - rows * cols:
        calls.append((1, 1, 1, count - rows * cols, 4 * rows * cols))
    return calls


def launch_arms(case):
    """[(arm, work items of the launch)] for every launch the case makes."""
    if case.op not in TV_OPS:
        if case.op == "batch_reduce":
            return [("plain", case.h * case.w * case.c)]  # per-sample elements; blocks own 64 of them
        if case.op == "im2col_strided":  # one item per output channel up to max(out.cpad, out.c)
            n, h, w, c = views(case)["out"]
            return [("plain", n * h * w * max(c, case.p[3]))]
        v = views(case)
        return [("plain", max(a * b * c_ * d for a, b, c_, d in v.values()))]
    if case.flat_axpy:
        out = []
        for n, h, w, c, boff in flat_axpy_calls(case.n * case.h * case.w * case.c):
            lay = (boff, h * w * c, w * c, c)
            if axpby_flat(4, n, h, w, c, NO_SPLIT, [lay, lay]):
                out.append(("flat", n * h * w * c // 4))
            elif vec4_ok(4, c, [lay, lay]):
                out.append(("vec", n * h * w * c // 4))
            else:
                out.append(("scalar", n * h * w * c))
        return out
    v = views(case)
    lays = [view_layout(case, s) for s in v.values()]
    n, h, w, c = v["out"]
    if case.op == "axpby":
        _a, _b, c_from, _fill = case.p
        if axpby_flat(case.esz, n, h, w, c, c_from, lays):
            return [("flat", n * h * w * c * case.esz // 16)]
    if vec4_ok(case.esz, c, lays):
        return [("vec", n * h * w * c // 4)]
    return [("scalar", n * h * w * c)]


def arm(case):
    return "+".join(a for a, _ in launch_arms(case))


def wraps(case):
    """More work items than one pass of the capped grid covers."""
    cap = BATCH_REDUCE_CAP if case.op == "batch_reduce" else GRID_CAP
    return any(items > cap for _, items in launch_arms(case))


# ----------------------------------------------------------------------------------------------------------------- the table
# layouts: (c, off, cext, pad) -> vector on a whole tensor, vector on a slice at offset 4 (its neighbours must survive the
# 4-channel stores), scalar by c % 4, scalar by a channel offset of 1, 2, 3
_LAYOUTS = [(8, 0, 0, 0), (8, 4, 4, 1), (5, 0, 0, 0), (13, 0, 3, 1), (8, 1, 3, 0), (8, 2, 2, 1), (8, 3, 1, 0)]


def _tv_params(op, big=False):
    """[(h, w, p)] of the op at the odd default size (7 x 5 outputs) or at a grid-wrapping size."""
    if op == "avgpool_fwd":
        return [(7, 5, (2,)), (3, 5, (3,))] if not big else [(128, 128, (2,))]
    if op == "avgpool_bwd":
        return [(14, 10, (2,)), (9, 6, (3,))] if not big else [(128, 128, (2,))]
    if op == "adaptive_avgpool_fwd":
        return [(7, 5, (12, 9)), (6, 4, (10, 7))] if not big else [(128, 128, (192, 192))]
    if op == "adaptive_avgpool_bwd":
        return [(12, 9, (7, 5)), (10, 7, (6, 4))] if not big else [(192, 192, (128, 128))]
    if op == "upsample_fwd":
        return [(14, 10, (7, 5, 1)), (7, 5, (1, 1, 1)), (12, 15, (4, 6, 0)), (9, 5, (3, 5, 1))] if not big else [(128, 128, (64, 64, 1))]
    if op == "upsample_bwd":
        return [(7, 5, (14, 10)), (1, 1, (7, 5)), (4, 6, (12, 15)), (3, 5, (9, 5))] if not big else [(128, 128, (256, 256))]
    if op == "batch_broadcast":
        return [(7, 5, ())] if not big else [(128, 128, ())]
    if op == "axpby":  # (alpha, beta, c_from, fill): c_from 2 and 6 fall inside a 4-channel group
        return [(7, 5, (1.5, 1.0, NO_SPLIT, 0)), (7, 5, (1.5, -0.75, 6, 0)), (7, 5, (0.5, 0.25, 2, 0)), (7, 5, (-2.5, 1.0, NO_SPLIT, 1))] \
            if not big else [(128, 128, (1.25, 0.5, 6, 0))]
    raise KeyError(op)


def build_cases():
    cases = []
    for op in TV_OPS:
        accs = (0, 1) if op in ACC_OPS else (0,)
        for dt in DTYPES:
            for li, (c, off, cext, pad) in enumerate(_LAYOUTS):
                for pi, (h, w, p) in enumerate(_tv_params(op)):
                    for acc in accs:
                        if (li + pi + acc) % 2 and pi > 0 and op != "axpby":  # thin the cross product; every layout still sees every acc
                            continue
                        cases.append(Case(op, dt, 3, h, w, c, off, cext, pad, acc, p))
        # more work items than the capped grid covers (> 2^20 at >= 2 x 128 x 128 outputs), in each arm: vector with 132 channels
        # (33 groups), scalar with 33 channels; the dtypes alternate between the arms from one entry point to the next
        oi = TV_OPS.index(op)
        for (h, w, p) in _tv_params(op, big=True):
            acc = 1 if op in ACC_OPS else 0
            cases.append(Case(op, DTYPES[oi % 2], 2, h, w, 132, 0, 0, 0, acc, p))
            cases.append(Case(op, DTYPES[1 - oi % 2], 2, h, w, 33, 0, 0, 0, acc, p))
        if op == "axpby":
            for dt in DTYPES:
                for acc in (0, 1):
                    cases.append(Case(op, dt, 3, 7, 5, 16, acc=acc, p=(1.5, 1.0, NO_SPLIT, 0)))  # whole contiguous: flat path
                    cases.append(Case(op, dt, 3, 7, 5, 16, acc=acc, p=(-0.5, 1.0, NO_SPLIT, 1)))  # flat fill
                cases.append(Case(op, dt, 4, 256, 256, 40, acc=1, p=(0.75, 1.0, NO_SPLIT, 0)))  # flat, > 2^20 16-byte vectors
            # Engine.flat_axpy: rows of 1024 (flat) + a tail that is flat (c % 4 == 0) or scalar; the last one wraps the grid
            for count, acc in ((3 * 1024 + 5, 1), (2 * 1024 + 12, 0), (1024 * 4200 + 13, 1), (7, 0)):
                cases.append(Case(op, "f32", 1, 1, 1, count, acc=acc, p=(1.25, 1.0, NO_SPLIT, 0), flat_axpy=True))
    for dt in DTYPES:
        for (n, h, w, c, off, cext, acc, unscale) in ((3, 7, 5, 8, 0, 0, 0, 1.0), (5, 7, 5, 5, 1, 2, 1, 0.25),
                                                      (1, 3, 3, 4, 3, 1, 0, 0.125), (9, 7, 5, 12, 0, 4, 1, 3.0),
                                                      (3, 64, 64, 72, 0, 0, 1, 0.0625), (2, 64, 65, 65, 2, 1, 0, 1.0)):
            cases.append(Case("batch_reduce", dt, n, h, w, c, off, cext, 1 if off else 0, acc, (unscale,)))
        for (n, h, w, c, off, cext, src, sub, mul) in ((3, 7, 5, 3, 0, 0, "f32", 0.0, 1.0), (3, 7, 5, 5, 2, 1, "f32", 0.5, -1.75),
                                                       (2, 9, 4, 8, 0, 0, "u8", 127.5, 1 / 127.5), (2, 6, 5, 3, 1, 0, "u8", 0.0, 1.0),
                                                       (4, 128, 128, 17, 0, 0, "f32", -0.25, 3.0)):
            cases.append(Case("nchw_to_nhwc", dt, n, h, w, c, off, cext, 1 if off else 0, 0, (src, sub, mul)))
        for (n, h, w, c, off, cext) in ((3, 7, 5, 3, 0, 0), (3, 7, 5, 8, 1, 3), (4, 128, 128, 17, 0, 0)):
            cases.append(Case("nhwc_to_nchw", dt, n, h, w, c, off, cext, 1 if off else 0))
        for (n, h, w, c, ks, cpad, off) in ((3, 7, 5, 1, 3, 0, 0), (3, 9, 7, 3, 5, 80, 0), (2, 11, 9, 4, 3, 40, 1),
                                            (2, 8, 8, 2, 5, 0, 2), (9, 129, 127, 3, 3, 32, 0)):
            cases.append(Case("im2col_strided", dt, n, h, w, c, off, 1 if off else 0, 1 if off else 0, 0, (ks, 2, 1, cpad)))
        for (n, h, w, c, ks, off, acc) in ((3, 7, 5, 1, 3, 0, 0), (3, 9, 7, 3, 5, 0, 1), (2, 11, 9, 4, 3, 1, 1),
                                           (2, 8, 8, 2, 5, 2, 0), (2, 10, 10, 3, 3, 0, 1), (4, 255, 257, 5, 3, 0, 1)):
            cases.append(Case("col2im_strided", dt, n, h, w, c, off, 1 if off else 0, 1 if off else 0, acc, (ks, 2, 1)))
        for u in UNARY:
            param = {"relu": 0.0, "gelu": 0.0, "leaky_relu": 0.1, "clamp_min": -0.375, "add": 0.7}[u]  # (min exact in 16 bits: x == min is reachable)
            for (n, h, w, c, off, cext) in ((3, 7, 5, 8, 0, 0), (3, 7, 5, 5, 3, 1), (4, 160, 160, 11, 0, 0)):
                cases.append(Case("unary_fwd", dt, n, h, w, c, off, cext, 1 if off else 0, 0, (u, param)))
                for acc in (0, 1):
                    cases.append(Case("unary_bwd", dt, n, h, w, c, off, cext, 1 if off else 0, acc, (u, param)))
    return cases


CASES = build_cases()
