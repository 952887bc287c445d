"""Case tables of the latent (csrc/latent.hip), likelihood and ELBO (csrc/likelihood.hip) kernels, shared by
tests/test_gpu_latent_like.py (runs each case against the f64 references of tests/latent_like_ref.py) and
tests/test_latent_like_cases.py (checks, without a GPU, that the tables reach every arm and every boundary the kernels have).

Every NHWC view of a case lies in a parent tensor [n + pad, h + pad, w + pad, off + c + cext] at channel offset `off`; the parent is
allocated whole (its base is at least 256-byte aligned), so the byte alignment of a view is `off * esz`.  `arm()` mirrors the
host-side choice of the latent kernels' instance (lat_vec8_ok of latent.hip): f32, h16-scalar or h16-vec8."""
import math
from dataclasses import dataclass, field

LAT_CHUNK = 2048  # per-sample elements of one reparam_kl_fwd block
LIKE_PIX = 1024  # pixels of one *_nll_fwd block
GRID_CAP = 4096 * 256  # lat_grid / like_grid: at most 4096 blocks of 256 threads, then the grid-stride loop wraps
DTYPES = ("f32", "h16")
LOGT = math.log(0.8)

LATENT_OPS = ("reparam_kl_fwd", "reparam_kl_bwd", "reparam_kl_bwd_rider", "sample_gaussian", "mediator_mix", "kl_channel_sums",
              "gaussian_kl_map")
LIKE_OPS = ("dgauss_nll_fwd", "dgauss_nll_bwd", "dgauss_params", "dgauss_sample", "cf_dgauss_bwd", "gauss_nll_fwd", "gauss_nll_bwd",
            "dmol_nll_fwd", "dmol_nll_bwd")
ELBO_OPS = ("elbo_finalize", "elbo_finalize_fb")
VEC8_OPS = ("reparam_kl_fwd", "reparam_kl_bwd")  # instance chosen per call by lat_vec8_ok
# the tolerance family of an entry point: one measured K each (tests/test_gpu_latent_like.py)
FAMILY = {"reparam_kl_fwd": "latent", "reparam_kl_bwd": "latent", "reparam_kl_bwd_rider": "latent", "sample_gaussian": "latent",
          "mediator_mix": "latent", "kl_channel_sums": "latent", "gaussian_kl_map": "latent",
          "dgauss_nll_fwd": "dgauss", "dgauss_nll_bwd": "dgauss", "dgauss_params": "dgauss", "dgauss_sample": "dgauss",
          "cf_dgauss_bwd": "dgauss", "gauss_nll_fwd": "gauss", "gauss_nll_bwd": "gauss",
          "dmol_nll_fwd": "dmol", "dmol_nll_bwd": "dmol", "elbo_finalize": "elbo", "elbo_finalize_fb": "elbo"}


@dataclass(frozen=True)
class Case:
    op: str
    dt: str  # "f32" or "h16" (the library's 16-bit format, cgen_h16_format())
    n: int
    h: int
    w: int
    c: int  # latent family: channels of every view; likelihood family: image channels C; ELBO: unused
    off: int = 0  # channel offset of every latent view / of the parameter view in its parent
    cext: int = 0  # parent channels after the view
    pad: int = 0  # parent rows / columns / samples beyond the view
    p: tuple = field(default_factory=tuple)  # ((name, value), ...) op parameters

    @property
    def esz(self):
        return 4 if self.dt == "f32" else 2

    def get(self, name, default=None):
        return dict(self.p).get(name, default)

    def id(self):
        s = f"{self.op}-{self.dt}-{arm(self)}-n{self.n}x{self.h}x{self.w}x{self.c}"
        if self.off or self.cext:
            s += f"-off{self.off}+{self.cext}"
        if self.pad:
            s += f"-pad{self.pad}"
        for k, v in self.p:
            s += f"-{k}{v:.3g}" if isinstance(v, float) else f"-{k}{v}"
        return s


def P(**kw):
    return tuple(kw.items())


# ------------------------------------------------------------------------------------------------------------- layout, arms
def param_channels(case):
    """Channels of the likelihood family's parameter view."""
    if case.op.startswith("dmol"):
        return 100
    return case.get("pc", 2 * case.c)


def view_channels(case, role):
    """Channels of the view `role` of a case: the latent family's views all have c; 'params' / 'g' of the likelihood family have the
    parameter channels, 'x' / 'u' the image channels; the rider's views have its own width."""
    if role in ("params", "g", "cf", "g_cf"):
        return param_channels(case)
    if role in ("ride_src", "ride_dst"):
        return case.get("ride_c")
    return 3 if case.op.startswith("dmol") else case.c


def parent_shape(case, shape):
    """(parent shape, channel offset) of a view of `shape`.  Views of the case's main width (latent: c; likelihood: the parameter
    channels) carry off / cext; the others (x, u, the rider) lie at offset 0 of a parent of their own width."""
    n, h, w, c = shape
    main = param_channels(case) if case.op in LIKE_OPS else case.c
    if c == main:
        return (n + case.pad, h + case.pad, w + case.pad, case.off + c + case.cext), case.off
    return (n + case.pad, h + case.pad, w + case.pad, c), 0


def view_layout(case, shape):
    """(byte offset from the parent base, sn, sh, sw) in elements, as torch slicing of the parent gives them."""
    (_, hp, wp, cp), off = parent_shape(case, shape)
    return off * case.esz, hp * wp * cp, wp * cp, cp


def lat_vec8_ok(n, c, layouts):
    """latent.hip lat_vec8_ok (16-bit only): channels a multiple of 8, base and every stride of every view a multiple of 16 bytes
    (vec16_ok with esz 2), and n * sn inside 31 bits."""
    if c % 8:
        return False
    for p, sn, sh, sw in layouts:
        if p % 16 or (sn * 2) % 16 or (sh * 2) % 16 or (sw * 2) % 16:
            return False
        if n * sn >= 1 << 31:
            return False
    return True


def arm(case):
    if case.dt == "f32":
        return "f32"
    if case.op in VEC8_OPS or case.op == "reparam_kl_bwd_rider":
        lay = view_layout(case, (case.n, case.h, case.w, case.c))
        return "h16-vec8" if lat_vec8_ok(case.n, case.c, [lay]) else "h16-scalar"
    return "h16"


def arms_of(op):
    if op in VEC8_OPS:
        return {"f32", "h16-scalar", "h16-vec8"}
    if op == "reparam_kl_bwd_rider":
        return {"h16-vec8"}  # (the rider exists in the 8-channel kernel only)
    if op in ELBO_OPS or op == "gaussian_kl_map":
        return {"f32"}
    return {"f32", "h16"}


def per(case):
    return case.h * case.w * case.c


def lat_chunks(case):
    return -(-per(case) // LAT_CHUNK)


def like_chunks(case):
    return -(-(case.h * case.w) // LIKE_PIX)


def work_items(case):
    """Items of the case's grid-stride launch (latent bwd: elements, or 8-channel groups in the vec8 arm; likelihood bwd: pixels)."""
    if case.op in ("reparam_kl_bwd", "reparam_kl_bwd_rider"):
        return case.n * per(case) // (8 if arm(case) == "h16-vec8" else 1)
    if case.op in ("sample_gaussian", "mediator_mix"):
        return case.n * per(case)
    if case.op == "gaussian_kl_map":
        return case.c
    if case.op in LIKE_OPS and not case.op.endswith("nll_fwd"):
        return case.n * case.h * case.w
    return 0  # (one block per chunk / per sample: no grid-stride loop)


def wraps(case):
    return work_items(case) > GRID_CAP


# ----------------------------------------------------------------------------------------------------------------- the tables
# (h, w, c) reaching per = 1, 2047, 2048, 2049 and 4920 = two whole chunks and a part
_PER_SHAPES = [(1, 1, 1), (23, 89, 1), (16, 16, 8), (1, 683, 3), (5, 41, 24)]
# (c, off, cext): 16-bit scalar arm by c % 8 (3, 12) and by 8-byte alignment (16 channels at offset 4); vec8 arm whole and on slices
_SCALAR_LAYOUTS = [(3, 0, 0), (12, 0, 4), (16, 4, 4)]
_VEC8_LAYOUTS = [(8, 0, 0), (16, 8, 8), (24, 0, 8), (16, 0, 0), (8, 8, 0)]
_PIX_SHAPES = [(1, 1), (33, 31), (32, 32), (25, 41), (45, 47)]  # 1, 1023, 1024, 1025, 2115 pixels


def _latent_cases():
    cs = []
    for dt in DTYPES:
        # ---- reparam_kl_fwd: the chunk boundaries, then the layouts of both 16-bit arms
        i = 0
        for (h, w, c) in _PER_SHAPES:
            for n in (1, 3):
                cs.append(Case("reparam_kl_fwd", dt, n, h, w, c, p=P(eps_out=i % 2, logt=LOGT if i % 3 == 0 else 0.0)))
                i += 1
        for (c, off, cext) in _SCALAR_LAYOUTS + _VEC8_LAYOUTS:
            for eps_out in (0, 1):
                cs.append(Case("reparam_kl_fwd", dt, 3, 7, 5, c, off, cext, 1, P(eps_out=eps_out, logt=0.0 if eps_out else LOGT)))
        # ---- reparam_kl_bwd: the same shapes; (gz, chan_scale, coef_stride, acc_q, acc_p) thinned so that every layout sees every
        # value of every argument, and all four (acc_q, acc_p) pairs meet both values of every other argument in each arm
        i = 0
        for (h, w, c) in _PER_SHAPES:
            for n in (1, 3):
                cs.append(Case("reparam_kl_bwd", dt, n, h, w, c,
                               p=P(gz=i % 2, cs=(i // 2) % 2, coef_stride=(i + 1) % 2, acc_q=(i // 2) % 2, acc_p=i % 2, logt=LOGT if i % 3 else 0.0)))
                i += 1
        for li, (c, off, cext) in enumerate(_SCALAR_LAYOUTS + _VEC8_LAYOUTS):
            for j in range(4):
                acc_q, acc_p = j // 2, j % 2
                for gz in (0, 1):
                    k = li + j + gz
                    cs.append(Case("reparam_kl_bwd", dt, 3, 7, 5, c, off, cext, 1,
                                   P(gz=gz, cs=(k // 2) % 2, coef_stride=k % 2, acc_q=acc_q, acc_p=acc_p, logt=LOGT if k % 3 else 0.0)))
        for (h, w, c) in ((7, 5, 8), (3, 3, 3)):
            for t in (0.0, 0.7):
                cs.append(Case("sample_gaussian", dt, 3, h, w, c, 0, 0, 1, P(logt=math.log(t) if t else 0.0)))
        # mediator_mix: simple_vae's 1 x 1 use and a spatial one
        for (n, h, w, c, off, cext) in ((5, 1, 1, 16, 0, 0), (3, 7, 5, 12, 2, 2)):
            for lv in (0, 1):
                for alpha in (0.0, 0.3, 1.0):
                    for t in (0.0, 0.7):
                        cs.append(Case("mediator_mix", dt, n, h, w, c, off, cext, 1 if off else 0, P(linear_var=lv, alpha=alpha, t=t)))
        # kl_channel_sums: a thread owns pixels slot, slot + L, ... with L = 256 / c lanes per channel
        for c in (1, 2, 16, 64, 256):
            L = 256 // c
            for hw in sorted({1, L - 1, L + 1, 3 * L + 1}):
                if hw > 0:
                    h, w = (1, hw) if hw % 3 else (3, hw // 3)
                    cs.append(Case("kl_channel_sums", dt, 3, h, w, c, 0, 0, 1, P(out_extra=3, logt=LOGT if hw % 2 else 0.0)))
    # grid wrap, one case per arm: more items than 4096 * 256
    wrap = P(gz=1, cs=1, coef_stride=1, acc_q=1, acc_p=0, logt=LOGT)
    cs.append(Case("reparam_kl_bwd", "f32", 3, 60, 61, 96, p=wrap))
    cs.append(Case("reparam_kl_bwd", "h16", 3, 60, 61, 100, p=wrap))  # (c % 8: the scalar 16-bit arm)
    cs.append(Case("reparam_kl_bwd", "h16", 2, 128, 129, 256, p=wrap))  # vec8: items are groups of 8 channels
    for (rc, acc, gz) in ((8, 0, 1), (8, 1, 0), (32, 0, 0), (32, 1, 1)):
        cs.append(Case("reparam_kl_bwd_rider", "h16", 3, 7, 5, 16, 0, 0, 1,
                       P(gz=gz, cs=acc, coef_stride=1 - acc, acc_q=acc, acc_p=1 - acc, logt=0.0, ride_c=rc, ride_acc=acc)))
    for count in (0, 1, 255, 257, GRID_CAP + 3):
        cs.append(Case("gaussian_kl_map", "f32", 1, 1, 1, count))
    return cs


def _like_cases():
    cs = []
    for dt in DTYPES:
        i = 0
        for (h, w) in _PIX_SHAPES:
            for n in (1, 3):
                # (C, pc, off, cext): grey; RGB autoregressive; RGB independent; a channel slice of a wider parent
                for (C, pc, off, cext) in ((1, 2, 0, 0), (3, 9, 0, 0), (3, 6, 0, 0), (1, 2, 3, 1), (3, 9, 2, 5)):
                    if (h * w > 1100 or (h * w == 1 and n == 3)) and off:
                        continue
                    cs.append(Case("dgauss_nll_fwd", dt, n, h, w, C, off, cext, 1 if off else 0, P(pc=pc)))
                    cs.append(Case("dgauss_nll_bwd", dt, n, h, w, C, off, cext, 1 if off else 0, P(pc=pc, coef_stride=i % 2)))
                    i += 1
        for (C, pc) in ((1, 2), (3, 9)):
            for xg in (0, 1):
                cs.append(Case("dgauss_params", dt, 3, 7, 5, C, 1, 2, 1, P(pc=pc, x=xg, logt=LOGT)))
            cs.append(Case("dgauss_sample", dt, 3, 7, 5, C, 0, 0, 0, P(pc=pc)))
        cs.append(Case("dgauss_sample", dt, 3, 7, 5, 3, 0, 0, 0, P(pc=6)))
        for (n, h, w, C, pc) in ((3, 7, 5, 1, 2), (3, 7, 5, 3, 9), (2, 33, 31, 3, 12), (3, 7, 5, 3, 6)):
            cs.append(Case("cf_dgauss_bwd", dt, n, h, w, C, 0, 0, 0, P(pc=pc)))
        for (h, w) in _PIX_SHAPES:
            for n in (1, 3):
                for C in (1, 3):
                    if (n == 3) == (C == 3) or h * w in (1023, 1025):
                        cs.append(Case("gauss_nll_fwd", dt, n, h, w, C, 0, 0, 0, P()))
                        cs.append(Case("gauss_nll_bwd", dt, n, h, w, C, 1, 1, 1, P(coef_stride=n % 2 if n > 1 else 0)))
        for (n, h, w) in ((3, 1, 1), (1, 33, 31), (2, 25, 41)):
            for low in (0, 1):
                cs.append(Case("dmol_nll_fwd", dt, n, h, w, 3, 0, 0, 0, P(low_bit=low)))
                cs.append(Case("dmol_nll_bwd", dt, n, h, w, 3, 0, 0, 0, P(low_bit=low, coef_stride=low if n > 1 else 0)))
        # images that hold the directed pixels and nothing else (latent_like_ref._like_inputs: 9, 5 and 10 of them): a forward chunk
        # sum is bounded by the sum of its elements' bounds, which a thousand random pixels make wider than one pixel's wrong branch
        # (C = 1: the other channels of a directed pixel are random ones)
        cs.append(Case("dgauss_nll_fwd", dt, 1, 1, 9, 1, 0, 0, 0, P(pc=2, only=1)))
        cs.append(Case("dgauss_nll_bwd", dt, 1, 1, 9, 1, 0, 0, 0, P(pc=2, coef_stride=0, only=1)))
        cs.append(Case("gauss_nll_fwd", dt, 1, 1, 5, 1, 0, 0, 0, P(only=1)))
        cs.append(Case("gauss_nll_bwd", dt, 1, 1, 5, 1, 0, 0, 0, P(coef_stride=0, only=1)))
        for low in (0, 1):
            cs.append(Case("dmol_nll_fwd", dt, 1, 1, 10, 3, 0, 0, 0, P(low_bit=low, only=1)))
            cs.append(Case("dmol_nll_bwd", dt, 1, 1, 10, 3, 0, 0, 0, P(low_bit=low, coef_stride=0, only=1)))
    cs.append(Case("dgauss_nll_bwd", "f32", 5, 459, 457, 1, 0, 0, 0, P(pc=2, coef_stride=1)))  # more pixels than 4096 * 256
    return cs


def _elbo_cases():
    cs = []
    ns, nlls, kls = (1, 15, 16, 17, 33, 100), (1, 63, 64, 65, 130), (0, 1, 64, 200)
    # every value of every argument, and every n with a count on each side of the 64-lane stride
    for i, n in enumerate(ns):
        for j in range(3):
            cs.append(Case("elbo_finalize", "f32", n, 1, 1, 1,
                           p=P(nll_count=nlls[(i + 2 * j) % 5], kl_count=kls[(i + j) % 4], beta_dev=(i + j) % 2)))
    for n in (1, 8, 300):
        for k, ncol in enumerate((1, 255, 256, 257, 700)):
            cs.append(Case("elbo_finalize_fb", "f32", n, 1, 1, 1,
                           p=P(ncol=ncol, nll_count=(1, 3, 65)[(k + n) % 3], cols=("above", "below", "mixed")[(k + n) % 3], beta_dev=k % 2)))
    for ncol in (1, 257):
        cs.append(Case("elbo_finalize_fb", "f32", 8, 1, 1, 1, p=P(ncol=ncol, nll_count=2, cols="tie", beta_dev=0)))
    return cs


LATENT_CASES = _latent_cases()
LIKE_CASES = _like_cases()
ELBO_CASES = _elbo_cases()
CASES = LATENT_CASES + LIKE_CASES + ELBO_CASES
