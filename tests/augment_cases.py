"""Case table of cgen_batch_augment (csrc/augment.hip), shared by tests/test_gpu_augment.py (runs every case bit-exactly against a CPU
crop pushed through cgen_nchw_to_nhwc) and tests/test_augment_abi.py (checks, without a GPU, that the table reaches every store arm).

A case's output view lies in a flat parent buffer whose base is at least 256-byte aligned:
  packed  contiguous NHWC [n, r_h, r_w, c]
  rowpad  pixels contiguous (pixel stride c), row stride rounded up to 16 elements: 16-byte groups plus an element-wise row end
  padded  the engine's own tensors: pixel stride 8 with cpad = 8 (the launch writes zeros into channels [c, 8))
  slice   channels [1, 1 + c) of a [n, r_h, r_w, c + 3] tensor: the neighbours must come back untouched"""
import ctypes as C
from dataclasses import dataclass

N_DATA, N, CTX = 3, 7, 5
INDEX = (2, 0, 0, 1, 2, 2, 1)  # n = 7 rows of a 3-row data set: repeated rows

# (h0, w0, r_h, r_w, pad_x, pad_y)
GEOMS = ((5, 7, 6, 4, 2, 1), (28, 28, 32, 32, 4, 4), (8, 8, 8, 8, 0, 0),
         (4, 4, 4, 4, 6, 5),      # padding larger than the image: whole rows and columns of a crop are padding
         (9, 13, 9, 13, 3, 2))    # odd r_w * c: element-wise rows


@dataclass(frozen=True)
class Case:
    c: int
    geom: tuple
    hflip_p: float
    layout: str = "packed"

    def id(self):
        return f"c{self.c}-" + "x".join(str(v) for v in self.geom) + f"-p{self.hflip_p}-{self.layout}"

    def view(self, n=N):
        """(sn, sh, sw, channel offset, cpad, parent elements) of the output view."""
        _, _, r_h, r_w, _, _ = self.geom
        c = self.c
        if self.layout == "packed":
            sw, sh, off, cpad = c, r_w * c, 0, 0
        elif self.layout == "rowpad":
            sw, sh, off, cpad = c, (r_w * c + 15) // 16 * 16, 0, 0
        elif self.layout == "padded":
            sw, sh, off, cpad = 8, r_w * 8, 0, 8
        else:
            sw, sh, off, cpad = c + 3, r_w * (c + 3), 1, 0
        sn = r_h * sh
        return sn, sh, sw, off, cpad, n * sn


CASES = tuple(Case(c, g, p) for c in (1, 3) for g in GEOMS for p in (0.0, 1.0, 0.5)) + (
    Case(1, GEOMS[4], 0.5, "rowpad"), Case(3, GEOMS[0], 0.5, "rowpad"),
    Case(1, GEOMS[1], 0.5, "padded"), Case(3, GEOMS[0], 0.5, "padded"), Case(3, GEOMS[4], 1.0, "padded"),
    Case(1, GEOMS[0], 0.5, "slice"), Case(3, GEOMS[4], 0.5, "slice"), Case(3, GEOMS[1], 1.0, "slice"),
)


def make_args(case, dt, data, index, out_base, rng=None, draws_in=None, draws_out=None, pa_data=None, pa_out=None, n=N, n_data=N_DATA,
              ctx=CTX, sub=127.5, mul=1 / 127.5):
    """cgen_augment_args of a case; pointers are plain integers (device addresses, or fakes for the no-launch queries)."""
    from causal_gen_amd import _lib

    h0, w0, r_h, r_w, px, py = case.geom
    sn, sh, sw, off, cpad, _ = case.view(n)
    esz = 4 if dt == "f32" else 2
    a = _lib.AugmentArgs()
    a.dtype = _lib.F32 if dt == "f32" else _lib.F16
    a.n, a.c, a.h0, a.w0, a.r_h, a.r_w, a.pad_x, a.pad_y, a.ctx = n, case.c, h0, w0, r_h, r_w, px, py, ctx
    a.stream_id, a.hflip_p, a.sub, a.mul, a.n_data = _lib.STREAM_AUGMENT, case.hflip_p, sub, mul, n_data
    a.data, a.index, a.rng, a.draws_in, a.draws_out, a.pa_data, a.pa_out = data, index, rng, draws_in, draws_out, pa_data, pa_out
    a.out = _lib.View(out_base + off * esz, sn, sh, sw, case.c, cpad)
    return a


def arm_of(case, dt):
    from causal_gen_amd import _lib

    a = make_args(case, dt, 1 << 20, 2 << 20, 3 << 20, rng=4 << 20)
    return _lib.load().batch_augment_arm(C.byref(a))
