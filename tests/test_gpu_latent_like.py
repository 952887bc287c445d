"""The latent (csrc/latent.hip), likelihood and ELBO (csrc/likelihood.hip) kernels called through the C ABI on views over torch
tensors, against the f64 references of tests/latent_like_ref.py, over the case tables of tests/latent_like_cases.py: both dtypes,
the f32 / h16-scalar / h16-vec8 arms, channel-slice views, every optional argument, the 1024-pixel and 2048-element chunk ends,
grid-stride wrap, the ELBO kernels' wave and column strides, and values written onto the kernels' branches (edge bins, the -9 and
-7 clamps with their storage neighbours, the 1e-12 floors, DMoL's delta <= 1e-5 fallback, the free-bits tie).

Tolerances.  Data movement (eps_out, the rider without accumulation) and chan_mask are bit for bit.  An element result is held to
K * 2^-24 * A, with A the same computation on absolute values (down to the tanh-CDF: 0.5 (1 + |tanh|), and the first-order effect
of the roundings of its argument), plus, in 16 bits, one unit in the last place of the storage format at the reference (for an
accumulated gradient: at the sum).  K is not guessed: it is the largest deviation, in those units, of torch's own f32 evaluation of
the same formulas from the f64 reference over all cases of a family, measured on the CPU (latent_like_ref.measure_k;
tests/test_latent_like_cases.py keeps the record honest), times 4 for the device's own expf / logf / tanhf -- the margin DESIGN
grants the PGM kernels over torch's f32 run.  Measured: latent 10.8, dgauss (with the counterfactual step) 8.8, gauss 15.8, dmol
17.8; recorded, rounded up, as 11, 9, 16, 18.  A term on an active floor or clamp (the 1e-12 floor, the logit's tiny clamp) is a
constant and amplifies nothing.  Reduced outputs (chunk partials, channel sums, the three ELBO numbers) get the sum of
their elements' bounds plus k * 2^-24 * sum |term|, k the longest addition chain of the kernel's fixed tree.  Random elements within
a relative 1e-3 of a branch threshold are not compared (they must be finite); directed values always are.  A forward chunk is
bounded by the sum of its elements' bounds, and a thousand random pixels (the tails within four scales carry 2 / delta) make that
wider than one pixel's wrong branch: so each NLL has cases that hold the directed pixels alone (`only1`), whose chunk bound the
CPU module holds under a fifth of what a removed clamp or a moved floor changes.

The tie.  At a raw DMoL log-scale of exactly -7.0 the reference's discretized_mix_logistic_loss (run once on the CPU on a pixel
with a tied, dominant component) returns 0.0194415 for the log-scale gradient where it returns 0.0390115 one thousandth above the
clamp and 0 below: one half of the pass-through gradient (0.0388830), torch.max's rule for const_max.  dm_logprob returned 0 there
and oracle/dmol_ref.py all of it; both now follow the reference (pixels 4..7 of every dmol case).

Every output lives in a parent filled with NaN: what the call must not write is compared bit for bit after it, including the
kl_part slots beyond the chunk count and the `out` columns beyond c."""
import math

import pytest
import torch

import latent_like_cases as T
import latent_like_ref as R
from gpu_views import U32, Arena, _bits, _cdt, _ulp, assert_exact, cv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from causal_gen_amd import _lib

    return _lib.require_gpu()


def _compare(name, got, o, k_fam, tdt):
    assert torch.isfinite(got).all(), f"{name}: not finite"
    ref = o.ref
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if o.exact:
        if o.excl is not None:
            keep = ~o.excl
            assert torch.equal(got[keep], ref.to(got.dtype)[keep]), name
        else:
            assert_exact(got, ref.to(got.dtype))
        return
    tol = k_fam * U32 * o.A
    if o.S is not None:
        tol = tol + U32 * o.S
    if o.loose is not None:
        tol = tol + o.loose
    if o.storage:
        tol = tol + _ulp(ref, tdt)
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)
    if o.excl is not None and o.loose is None:
        bad &= ~o.excl.bool()
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.numel()} outside the K={k_fam} bound; worst err/tol "
                           f"{float((err / tol.clamp_min(1e-300))[bad].max()):.3g}; first at {bad.nonzero()[0].tolist()}; got "
                           f"{got.double()[bad][:4].tolist()} want {ref[bad][:4].tolist()}")


class Run:
    """The views and flat buffers of one case, filled from the case's stored inputs."""

    def __init__(self, lib, case):
        self.lib, self.case = lib, case
        self.A = Arena(lib, case, T.parent_shape)
        self.tdt = self.A.tdt
        self.inp = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in R.make_inputs(case, self.tdt).items()}
        self.st = torch.cuda.current_stream().cuda_stream
        self.flats = []

    def vin(self, name):
        t = self.inp[name]
        v = self.A.view(tuple(t.shape))
        v.copy_(t)
        return v

    def vout(self, shape, init=None):
        v = self.A.view(tuple(shape), out=True, init=False)
        if init is not None:
            v.copy_(self.inp[init])
        return v

    def flat(self, count):
        """A contiguous NaN-filled f32 destination (+ 64 sentinels); `written` marks what the call may write."""
        buf = torch.full((count + 64,), float("nan"), device="cuda")
        self.flats.append((buf, buf.clone(), torch.zeros(count + 64, dtype=torch.bool, device="cuda")))
        return buf[:count], self.flats[-1][2][:count]

    def dev(self, name):
        return self.inp[name].contiguous()

    def check_untouched(self):
        self.A.check_untouched()
        for buf, before, written in self.flats:
            assert torch.equal(_bits(buf)[~written], _bits(before)[~written]), "a write outside the output"


def _run(lib, case):
    from causal_gen_amd import _lib

    r = Run(lib, case)
    dt, op, st, tdt = _cdt(case.dt), case.op, r.st, r.tdt
    n, h, w, c = case.n, case.h, case.w, case.c
    NV = _lib.NULL_VIEW
    got = {}
    if op in ("reparam_kl_fwd", "reparam_kl_bwd", "reparam_kl_bwd_rider", "sample_gaussian", "mediator_mix", "kl_channel_sums"):
        ql, qs, pl, ps = (r.vin(k) for k in ("q_loc", "q_ls", "p_loc", "p_ls"))
        sh = (n, h, w, c)
        if T.arm(case) == "h16-vec8":  # the mirror's verdict holds for the views actually built
            assert all(v.data_ptr() % 16 == 0 and all(s * 2 % 16 == 0 for s in v.stride()[:3]) for v in (ql, qs, pl, ps))
    if op == "reparam_kl_fwd":
        nch = lib.reparam_kl_chunks(h, w, c)
        assert nch == T.lat_chunks(case)
        stride = nch + 3  # sentinel slots between the samples
        eps, z = r.vin("eps"), r.vout(sh)
        eo = r.vout(sh) if case.get("eps_out") else None
        part, wr = r.flat(n * stride)
        wr.view(n, stride)[:, :nch] = True
        lib.reparam_kl_fwd(dt, n, h, w, c, cv(ql), cv(qs), cv(pl), cv(ps), cv(eps), None, 0, case.get("logt"), cv(z),
                           cv(eo) if eo is not None else NV, part.data_ptr(), stride, st)
        got = {"z": z, "kl_part": part.view(n, stride)[:, :nch]}
        if eo is not None:
            got["eps_out"] = eo
    elif op in ("reparam_kl_bwd", "reparam_kl_bwd_rider"):
        has_gz = case.get("gz")
        z, gz = (r.vin("z"), r.vin("gz")) if has_gz else (None, None)
        coef, cs = r.dev("coef"), r.dev("chan_scale")
        names = ("g_q_loc", "g_q_ls", "g_p_loc", "g_p_ls")
        outs = [r.vout(sh, init=k if case.get("acc_q" if j < 2 else "acc_p") else None) for j, k in enumerate(names)]
        args = [dt, n, h, w, c, cv(ql), cv(qs), cv(pl), cv(ps), cv(z) if has_gz else NV, case.get("logt"), cv(gz) if has_gz else NV,
                coef.data_ptr(), case.get("coef_stride"), cs.data_ptr() if case.get("cs") else None] + [cv(o) for o in outs] + \
               [case.get("acc_q"), case.get("acc_p")]
        got = dict(zip(names, outs))
        if op == "reparam_kl_bwd":
            lib.reparam_kl_bwd(*args, st)
        else:
            src = r.vin("ride_src")
            dst = r.vout(src.shape, init="ride_dst" if case.get("ride_acc") else None)
            lib.reparam_kl_bwd_rider(*args, cv(src), cv(dst), case.get("ride_acc"), st)
            got["ride_dst"] = dst
    elif op == "sample_gaussian":
        eps, z = r.vin("eps"), r.vout(sh)
        lib.sample_gaussian(dt, n, h, w, c, cv(ql), cv(qs), cv(eps), None, 0, case.get("logt"), cv(z), st)
        got = {"z": z}
    elif op == "mediator_mix":
        z, out = r.vin("z"), r.vout(sh)
        t = case.get("t")
        lib.mediator_mix(dt, n, h, w, c, cv(z), cv(ql), cv(qs), cv(pl), cv(ps), case.get("alpha"), t, math.log(t) if t > 0 else 0.0,
                         case.get("linear_var"), cv(out), st)
        got = {"out": out}
    elif op == "kl_channel_sums":
        stride = c + case.get("out_extra")
        out, wr = r.flat(n * stride)
        wr.view(n, stride)[:, :c] = True
        lib.kl_channel_sums(dt, n, h, w, c, cv(ql), cv(qs), cv(pl), cv(ps), case.get("logt"), out.data_ptr(), stride, st)
        got = {"out": out.view(n, stride)[:, :c]}
    elif op == "gaussian_kl_map":
        out, wr = r.flat(c)
        wr[:] = True
        a = [r.dev(k) for k in ("q_loc", "q_ls", "p_loc", "p_ls")]
        ptrs = [t.data_ptr() for t in a] + [out.data_ptr()]
        if c == 0:  # (an empty tensor has no address; the call wants non-null pointers and must touch none of them)
            ptrs = [r.flats[0][0].data_ptr()] * 5
        lib.gaussian_kl_map(c, *ptrs, st)
        got = {"out": out}
    elif op in T.LIKE_OPS:
        C = case.c
        params, x = r.vin("params"), r.vin("x")
        nch = lib.like_chunks(h, w)
        assert nch == T.like_chunks(case)
        low = _lib.DMOL_LOW_BIT if case.get("low_bit") else 0
        if op.endswith("nll_fwd"):
            part, wr = r.flat(n * nch)
            wr[:] = True
            if op == "dgauss_nll_fwd":
                lib.dgauss_nll_fwd(dt, n, h, w, C, cv(params), cv(x), part.data_ptr(), st)
            elif op == "gauss_nll_fwd":
                lib.gauss_nll_fwd(dt, n, h, w, C, cv(params), cv(x), cv(r.vin("u")), None, 0, part.data_ptr(), st)
            else:
                lib.dmol_nll_fwd(dt | low, n, h, w, cv(params), cv(x), part.data_ptr(), st)
            got = {"nll_part": part.view(n, nch)}
        elif op in ("dgauss_nll_bwd", "gauss_nll_bwd", "dmol_nll_bwd"):
            coef, g = r.dev("coef"), r.vout(params.shape)
            if op == "dgauss_nll_bwd":
                lib.dgauss_nll_bwd(dt, n, h, w, C, cv(params), cv(x), coef.data_ptr(), case.get("coef_stride"), cv(g), st)
            elif op == "gauss_nll_bwd":
                lib.gauss_nll_bwd(dt, n, h, w, C, cv(params), cv(x), cv(r.vin("u")), None, 0, coef.data_ptr(), case.get("coef_stride"), cv(g), st)
            else:
                lib.dmol_nll_bwd(dt | low, n, h, w, cv(params), cv(x), coef.data_ptr(), case.get("coef_stride"), cv(g), st)
            got = {"g": g}
        elif op in ("dgauss_params", "dgauss_sample"):
            (a, wa), (b, wb) = r.flat(n * C * h * w), r.flat(n * C * h * w)
            wa[:] = True
            wb[:] = True
            if op == "dgauss_params":
                lib.dgauss_params(dt, n, h, w, C, cv(params), cv(x) if case.get("x") else NV, case.get("logt"), a.data_ptr(), b.data_ptr(), st)
                got = {"loc": a.view(n, C, h, w), "ls": b.view(n, C, h, w)}
            else:
                lib.dgauss_sample(dt, n, h, w, C, cv(params), 0.0, None, 0, a.data_ptr(), b.data_ptr(), st)
                got = {"x": a.view(n, C, h, w), "scale": b.view(n, C, h, w)}
        elif op == "cf_dgauss_bwd":
            cf, gc = r.vin("cf"), r.dev("g_cfx")
            g_rec, g_cf = r.vout(params.shape), r.vout(params.shape)
            lib.cf_dgauss_bwd(dt, n, h, w, C, cv(params), cv(cf), cv(x), gc.data_ptr(), R.GSCALE, cv(g_rec), cv(g_cf), st)
            got = {"g": g_rec, "g_cf": g_cf}
            if T.param_channels(case) > 9:
                torch.cuda.synchronize()
                assert not g_rec[..., 9:].any() and not g_cf[..., 9:].any(), "channels 9.. of both gradients come back zero"
        else:
            raise KeyError(op)
    elif op in T.ELBO_OPS:
        nll = r.dev("nll_part")
        beta = r.inp["beta"]
        bdev = torch.tensor([beta], device="cuda") if case.get("beta_dev") else None
        by_value = 99.0 if bdev is not None else beta  # (beta_dev overrides the value)
        out3, w3 = r.flat(3)
        w3[:] = True
        if op == "elbo_finalize":
            kc = case.get("kl_count")
            kl = r.dev("kl_part")
            lib.elbo_finalize(n, nll.data_ptr(), case.get("nll_count"), R.NLL_DIV, kl.data_ptr() if kc else None, kc, R.KL_DIV, by_value,
                              bdev.data_ptr() if bdev is not None else None, out3.data_ptr(), st)
            got = {"out3": out3}
        else:
            ncol = case.get("ncol")
            mask, wm = r.flat(ncol)
            wm[:] = True
            lib.elbo_finalize_fb(n, nll.data_ptr(), case.get("nll_count"), R.NLL_DIV, r.dev("kl_bc").data_ptr(), ncol, R.KL_DIV, R.FREE_BITS,
                                 by_value, bdev.data_ptr() if bdev is not None else None, out3.data_ptr(), mask.data_ptr(), st)
            got = {"out3": out3, "chan_mask": mask}
    else:
        raise KeyError(op)

    torch.cuda.synchronize()
    ref = R.reference(case, r.inp)
    assert set(ref) == set(got), (set(ref), set(got))
    k_fam = R.K.get(T.FAMILY[op], 0.0)
    for name, o in ref.items():
        _compare(f"{case.id()}:{name}", got[name], o, k_fam, tdt)
    r.check_untouched()


@pytest.mark.parametrize("case", T.LATENT_CASES, ids=[c.id() for c in T.LATENT_CASES])
def test_latent(lib, case):
    _run(lib, case)


@pytest.mark.parametrize("case", T.LIKE_CASES, ids=[c.id() for c in T.LIKE_CASES])
def test_likelihood(lib, case):
    _run(lib, case)


@pytest.mark.parametrize("case", T.ELBO_CASES, ids=[c.id() for c in T.ELBO_CASES])
def test_elbo(lib, case):
    _run(lib, case)
