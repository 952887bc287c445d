"""Helpers shared by the GPU tests that call the C ABI on views over torch tensors (tests/test_gpu_elementwise.py,
tests/test_gpu_latent_like.py): dtype mapping, units in the last place, NaN-filled output parents whose untouched part is
compared bit for bit, and the two comparisons (exact; k * 2^-24 * the computation on absolute values + one storage ulp)."""
import zlib

import torch

U32 = 2.0 ** -24


def _tdt(lib, dt):
    return torch.float32 if dt == "f32" else (torch.bfloat16 if lib.h16_is_bf16 else torch.float16)


def _cdt(dt):
    from causal_gen_amd import _lib

    return _lib.F32 if dt == "f32" else _lib.F16


def f32(v):
    return torch.tensor(v, dtype=torch.float32).item()


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _ulp(x, tdt):
    """One unit in the last place of the output format at |x| (f32: none -- the k * 2^-24 term holds the final rounding)."""
    if tdt == torch.float32:
        return torch.zeros_like(x)
    mant, tiny = (10, 2.0 ** -24) if tdt == torch.float16 else (7, 2.0 ** -133)
    _, e = torch.frexp(x.abs())
    return torch.ldexp(torch.ones_like(x), (e - 1 - mant).to(x.dtype)).clamp_min(tiny)


class Arena:
    """Parents of the views of one case; output parents start as NaN so that stray writes show."""

    def __init__(self, lib, case, parent_shape):
        self.case = case
        self.parent_shape = parent_shape  # (case, view shape) -> (parent shape, channel offset)
        self.tdt = _tdt(lib, case.dt)
        self.g = torch.Generator(device="cuda").manual_seed(zlib.crc32(case.id().encode()))
        self.outs = []

    def rand(self, shape, dtype=torch.float32, scale=1.0):
        return (torch.randn(shape, generator=self.g, device="cuda") * scale).to(dtype)

    def view(self, shape, out=False, init=True, scale=1.0):
        (pn, ph, pw, pc), off = self.parent_shape(self.case, shape)
        n, h, w, c = shape
        if out:
            parent = torch.full((pn, ph, pw, pc), float("nan"), dtype=self.tdt, device="cuda")
        else:
            parent = self.rand((pn, ph, pw, pc), self.tdt, scale)
        assert parent.data_ptr() % 256 == 0  # (the alignment the case table's arm mirror assumes)
        v = parent[:n, :h, :w, off:off + c]
        if out:
            if init:
                v.copy_(self.rand(v.shape, self.tdt, scale))
            self.outs.append((parent, v, parent.clone()))
        return v

    def place(self, pshape, off, shape, values=None, out=False, zero_to=0, planes=1):
        """`planes` views of `shape` (n, h, w, c) at channel `off` of as many parents of `pshape`, one allocation, every parent filled
        with NaN: whatever a kernel takes from outside an input view shows in its result, and what it writes outside an output view
        shows in check_untouched.  `values`: one tensor per plane (any dtype; None leaves that view NaN).  Channels [c, zero_to) of the
        view's pixels hold zeros, as cgen_view.cpad promises.  Returns the views; the second one starts pn * sn elements after the first."""
        pn, ph, pw, pc = pshape
        n, h, w, c = shape
        whole = torch.full((planes * pn, ph, pw, pc), float("nan"), dtype=self.tdt, device="cuda")
        assert whole.data_ptr() % 256 == 0
        views = []
        for k in range(planes):
            parent = whole[k * pn:(k + 1) * pn]
            if zero_to > c:
                parent[:n, :h, :w, off + c:off + zero_to] = 0
            v = parent[:n, :h, :w, off:off + c]
            if values is not None and values[k] is not None:
                v.copy_(values[k].to(self.tdt))
            if out:
                self.outs.append((parent, v, parent.clone()))
            views.append(v)
        return views

    def flat_out(self, count, init):
        """A contiguous f32 destination with 64 sentinel floats after it."""
        buf = torch.full((count + 64,), float("nan"), device="cuda")
        if init:
            buf[:count] = self.rand((count,))
        self.outs.append((buf, buf[:count], buf.clone()))
        return buf[:count]

    def check_untouched(self, written=None, cpad=0):
        """Everything outside the written region of every output parent is bit-identical to what it was (the region: the view, or
        `written`; `cpad` channels of it where the call also writes the zero padding [c, cpad) of an output view -- one number for
        every output, or one per output in the order they were made)."""
        for i, (parent, v, before) in enumerate(self.outs):
            cp = cpad[i] if isinstance(cpad, (list, tuple)) else cpad
            keep = torch.ones(parent.shape, dtype=torch.bool, device="cuda")
            if parent.dim() == 1:
                keep[:v.numel()] = False
            else:
                r = written if written is not None else v
                c0 = (r.data_ptr() - parent.data_ptr()) // parent.element_size() % parent.stride(2)
                keep[:r.shape[0], :r.shape[1], :r.shape[2], c0:c0 + max(r.shape[3], cp)] = False
            assert torch.equal(_bits(parent)[keep], _bits(before)[keep]), "a write outside the output view"


def cv(v, cpad=0):
    from causal_gen_amd import _lib

    assert v.stride(3) == 1
    return _lib.View(v.data_ptr(), v.stride(0), v.stride(1), v.stride(2), v.shape[3], cpad)


def assert_exact(got, ref):
    """Bit for bit up to the sign of zero; NaN exactly where the reference has NaN."""
    assert got.dtype == ref.dtype and got.shape == ref.shape
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), "NaN pattern differs"
    bad = (got != ref) & ~nan
    assert not bad.any(), f"{int(bad.sum())} elements differ, e.g. got {got[bad][:4].tolist()} want {ref[bad][:4].tolist()}"


def assert_bounded(got, ref64, abs64, k, tdt):
    tol = k * U32 * abs64 + _ulp(ref64, tdt)
    err = (got.double() - ref64).abs()
    bad = ~(err <= tol)
    assert not bad.any(), (f"{int(bad.sum())} of {bad.numel()} outside the k={k} bound; worst err/tol "
                           f"{float((err / tol.clamp_min(1e-300)).max()):.3g}; got {got.double()[bad][:4].tolist()} "
                           f"want {ref64[bad][:4].tolist()}")
