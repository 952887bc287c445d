"""f64 references of the latent, likelihood and ELBO kernels for the cases of tests/latent_like_cases.py, in plain torch.

`make_inputs(case, tdt)` draws the stored inputs of a case (CPU, seeded by the case id, already rounded to the storage dtype) and
writes the directed values; `reference(case, inp, dt)` evaluates the kernel's formulas on those stored inputs in `dt` (float64:
the reference; float32: torch's own single-precision run, from which the tolerance constant K of a family is measured) and
returns, per output, the value, its amplification A (the same computation on absolute values), the summation term of a reduced
output and the mask of elements next to a branch threshold.  Where oracle/ states the formula it is called; gradients come from
autograd.  Everything runs on the device the inputs are on."""
import math
import zlib
from dataclasses import dataclass

import torch
import torch.nn.functional as F

import latent_like_cases as T
from oracle import dmol_ref, hvae_ref, simple_ref

U32 = 2.0 ** -24
HB8, LOGC8 = 1.0 / 255.0, math.log(127.5)
HB5, LOGC5 = 1.0 / 31.0, math.log(15.5)
F32_TINY, F32_EPS = 1.17549435e-38, 1.1920929e-07  # torch's SigmoidTransform.inv clamp in f32: what gs_target uses
FREE_BITS = 0.25
NEAR = 1e-3  # relative distance from a branch threshold inside which a random element is not compared

# K per family: the largest deviation of torch's f32 evaluation of these formulas from the f64 one, in units of 2^-24 * A, over all
# cases of the family (measure_k below; recorded in LABNOTES), times 4 for the device's own expf / logf / tanhf.
K_MEASURED = {"latent": 11.0, "dgauss": 9.0, "gauss": 16.0, "dmol": 18.0}
K = {fam: 4.0 * k for fam, k in K_MEASURED.items()}


def f32(v):
    return torch.tensor(v, dtype=torch.float32).item()


def storage_ulp(tdt, at, below):
    """The neighbour of `at` in the storage format, one unit in the last place below / above it."""
    t = torch.tensor(at, dtype=tdt)
    return torch.nextafter(t, torch.tensor(-math.inf if below else math.inf, dtype=tdt)).item()


@dataclass
class Out:
    ref: torch.Tensor  # float64 (or `dt`) value of the whole output view
    A: torch.Tensor = None  # amplification of the f32 roundings, per element (a reduced output: the sum over its elements)
    S: torch.Tensor = None  # chain length * sum |term| of a reduced output (units of 2^-24)
    excl: torch.Tensor = None  # elements next to a branch threshold (never a directed one)
    exact: bool = False  # data movement: bit for bit
    storage: bool = True  # stored in the case's dtype (16 bits: one more ulp); False: an f32 output
    terms: tuple = None  # (term, A) per element of a reduced output: what K is measured on
    loose: torch.Tensor = None  # absolute allowance of a reduced output for the excluded elements it holds


def _gen(case):
    return torch.Generator().manual_seed(zlib.crc32(case.id().encode()))


def _randn(g, shape, tdt, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(tdt)


def _unif(g, shape, lo, hi):
    return torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo


def _grid_x(g, shape):
    return (torch.randint(0, 256, shape, generator=g).double() - 127.5) / 127.5


# =============================================================================================================== inputs
def make_inputs(case, tdt):
    g = _gen(case)
    op = case.op
    inp = {}
    n, h, w, c = case.n, case.h, case.w, case.c
    sh = (n, h, w, c)
    if op in ("reparam_kl_fwd", "reparam_kl_bwd", "reparam_kl_bwd_rider", "sample_gaussian", "mediator_mix", "kl_channel_sums"):
        lt = f32(case.get("logt", 0.0))
        for k in ("q_loc", "p_loc"):
            inp[k] = _randn(g, sh, tdt)
        for k in ("q_ls", "p_ls"):
            inp[k] = _unif(g, sh, -3.0, 1.0).to(tdt)
        inp["eps"] = _randn(g, sh, tdt)
        if op.startswith("reparam_kl_bwd"):
            inp["z"] = (inp["q_loc"].double() + (inp["q_ls"].double() + lt).exp() * inp["eps"].double()).to(tdt)
            inp["gz"] = _randn(g, sh, tdt)
            inp["coef"] = (0.37 * (1.0 + torch.arange(n if case.get("coef_stride") else 1))).float()
            inp["chan_scale"] = torch.tensor([0.0, 0.5, 1.0])[torch.arange(c) % 3].float()
            for k in ("g_q_loc", "g_q_ls", "g_p_loc", "g_p_ls"):
                inp[k] = _randn(g, sh, tdt)
            if op.endswith("rider"):
                rs = (n, h, w, case.get("ride_c"))
                inp["ride_src"], inp["ride_dst"] = _randn(g, rs, tdt), _randn(g, rs, tdt)
        if op == "mediator_mix":
            inp["z"] = _randn(g, sh, tdt)
    elif op == "gaussian_kl_map":
        for k in ("q_loc", "p_loc"):
            inp[k] = torch.randn(c, generator=g)
        for k in ("q_ls", "p_ls"):
            inp[k] = _unif(g, (c,), -3.0, 1.0).float()
    elif op in T.LIKE_OPS:
        inp = _like_inputs(case, tdt, g)
    elif op == "elbo_finalize":
        nc, kc = case.get("nll_count"), case.get("kl_count")
        inp["nll_part"] = (torch.rand(n * nc, generator=g) * 5000.0 - 500.0).float()
        inp["kl_part"] = (torch.rand(n * kc, generator=g) * 40.0 - 2.0).float()
        inp["beta"] = 0.7
    elif op == "elbo_finalize_fb":
        nc, ncol, cols = case.get("nll_count"), case.get("ncol"), case.get("cols")
        inp["nll_part"] = (torch.rand(n * nc, generator=g) * 5000.0 - 500.0).float()
        hi, lo = torch.rand(n, ncol, generator=g) + 0.5, torch.rand(n, ncol, generator=g) * 0.1
        if cols == "tie":
            kl = torch.full((n, ncol), FREE_BITS)
        elif cols == "mixed":
            kl = torch.where((torch.arange(ncol) % 3 == 0)[None], lo, hi)
        else:
            kl = hi if cols == "above" else lo
        inp["kl_bc"] = kl.float().contiguous()
        inp["beta"] = 1.3
    else:
        raise KeyError(op)
    return inp


def _like_inputs(case, tdt, g):
    """Bulk: log-scales in [-3, 1], |x - loc| within four scales, x on the 8-bit grid; then the directed values, in the pixels
    0, 1, 2, ... of the flattened batch (as many as it has).  `directed` marks the pixels that hold one."""
    op, n, h, w, C = case.op, case.n, case.h, case.w, case.c
    pc = T.param_channels(case)
    npx = n * h * w
    inp = {}
    directed = torch.zeros(npx, dtype=torch.bool)

    def put(t, px, ch, v):
        if px < npx:
            t.view(npx, -1)[px, ch] = v
            directed[px] = True

    def same_as_pixel_4(t):  # pixels 4..7 differ in the directed log-scale only
        if npx >= 8:
            t.view(npx, -1)[5:8] = t.view(npx, -1)[4]

    if op.startswith("dmol"):
        hb = HB5 if case.get("low_bit") else HB8
        x = _grid_x(g, (n, h, w, 3))
        for j, v in enumerate((-1.0, 1.0, 1.0 - 2.0 / 255.0, -(1.0 - 2.0 / 255.0))):
            put(x, j, j % 3, v)
        for px in range(4, 10):
            put(x, px, 0, 4.5 / 127.5)
        same_as_pixel_4(x)
        x = x.to(tdt)
        xs = x.double()
        l = torch.zeros(n, h, w, 100, dtype=torch.float64)
        l[..., :10] = torch.randn(n, h, w, 10, generator=g, dtype=torch.float64)
        co_raw = (torch.randn(n, h, w, 3, 10, generator=g, dtype=torch.float64) * 0.5).to(tdt).double()
        ls = _unif(g, (n, h, w, 3, 10), -3.0, 1.0).to(tdt).double()
        mu = xs[..., None] + _unif(g, (n, h, w, 3, 10), -4.0, 4.0) * ls.exp()  # the autoregressive mean each component should have
        k = torch.tanh(co_raw)
        mean = mu.clone()
        mean[..., 1, :] -= k[..., 0, :] * xs[..., 0, None]
        mean[..., 2, :] -= k[..., 1, :] * xs[..., 0, None] + k[..., 2, :] * xs[..., 1, None]
        rest = torch.cat([mean, ls, co_raw], dim=-1)  # [n, h, w, 3, 30]
        l[..., 10:] = rest.reshape(n, h, w, 90)
        same_as_pixel_4(l)
        # pixels 4..7: component 0 carries the pixel, its R mean half a scale inside the lower bin edge, its raw R log-scale at the
        # clamp, one storage ulp below, one above, far below
        x0 = torch.tensor(4.5 / 127.5, dtype=tdt).double().item()
        for j, v in enumerate((-7.0, storage_ulp(tdt, -7.0, True), storage_ulp(tdt, -7.0, False), -20.0)):
            put(l, 4 + j, 0, 6.0)
            put(l, 4 + j, 10, x0 - hb + 0.5 * math.exp(-7.0))
            put(l, 4 + j, 20, v)
            if 4 + j < npx:  # its G and B: on the pixel at a scale of e^-3, so that the pixel's bound stays that of the R term
                xr, kr = xs.view(npx, 3)[4 + j], torch.tanh(co_raw.view(npx, 3, 10)[4, :, 0])
                put(l, 4 + j, 40, float(xr[1] - kr[0] * xr[0])), put(l, 4 + j, 50, -3.0)
                put(l, 4 + j, 70, float(xr[2] - kr[1] * xr[0] - kr[2] * xr[1])), put(l, 4 + j, 80, -3.0)
        # pixels 8, 9: every component's R mean ~ 70 scales from x: delta <= 1e-5, the log-density fallback decides the pixel
        for px in (8, 9):
            for m in range(10):
                put(l, px, 10 + m, x0 + 0.45 + 0.01 * m)
                put(l, px, 20 + m, -5.0)
        inp["x"], inp["params"] = x, l.to(tdt)
    elif op in ("gauss_nll_fwd", "gauss_nll_bwd"):
        x = _grid_x(g, (n, h, w, C))
        u = torch.rand(n, h, w, C, generator=g, dtype=torch.float64)
        put(x, 0, 0, -1.0)
        put(u, 0, 0, 0.0)
        ls = _unif(g, (n, h, w, C), -3.0, 1.0)
        x, u = x.to(tdt), u.to(tdt)
        v = (((x.double() + 1.0) * 127.5 + u.double()) / 256.0).clamp(min=F32_TINY, max=1.0 - F32_EPS)
        tgt = v.log() - (-v).log1p()
        loc = tgt + _unif(g, (n, h, w, C), -4.0, 4.0) * ls.exp()
        p = torch.cat([loc, ls], dim=-1)
        # pixels 1..4: the raw log-scale at the clamp, one storage ulp below, one above, far below; the mean sits on the target (as
        # near as the storage format resolves it: at a scale of e^-9 anything further overflows a 16-bit gradient)
        for j, val in enumerate((-9.0, storage_ulp(tdt, -9.0, True), storage_ulp(tdt, -9.0, False), -20.0)):
            put(p, 1 + j, C, val)
            if 1 + j < npx:
                put(p, 1 + j, 0, tgt.view(npx, -1)[1 + j, 0].item())
        inp["x"], inp["u"], inp["params"] = x, u, p.to(tdt)
    else:  # the discretised Gaussian head and its users
        x = _grid_x(g, (n, h, w, C))
        for j, v in enumerate((-1.0, 1.0, 1.0 - 2.0 / 255.0, -(1.0 - 2.0 / 255.0))):
            put(x, j, j % C, v)
        for px in range(4, 9):
            put(x, px, 0, 0.5 / 127.5)
        same_as_pixel_4(x)
        x = x.to(tdt)
        xs = x.double()
        ar = C == 3 and pc >= 9

        def head(beyond):
            ls = _unif(g, (n, h, w, C), -3.0, 1.0).to(tdt).double()
            kraw = (torch.randn(n, h, w, 3, generator=g, dtype=torch.float64) * 0.5).to(tdt).double()
            if beyond:  # raw locs beyond +-1, so that the clamps of the x-less decode act
                loc = _unif(g, (n, h, w, C), -1.6, 1.6)
            else:
                loc = xs + _unif(g, (n, h, w, C), -4.0, 4.0) * ls.exp()
                if ar:  # the mean the autoregressive form should reach, on the true pixels
                    k = torch.tanh(kraw)
                    loc[..., 1] -= k[..., 0] * xs[..., 0]
                    loc[..., 2] -= k[..., 1] * xs[..., 0] + k[..., 2] * xs[..., 1]
            parts = [loc, ls] + ([kraw] if ar else []) + [torch.randn(n, h, w, pc - 2 * C - (3 if ar else 0), generator=g, dtype=torch.float64)]
            return torch.cat(parts, dim=-1)

        beyond = op in ("dgauss_sample", "cf_dgauss_bwd") or (op == "dgauss_params" and not case.get("x"))
        p = head(beyond)
        same_as_pixel_4(p)
        x0 = torch.tensor(0.5 / 127.5, dtype=tdt).double().item()
        # pixels 4..7: x half a scale inside the lower bin edge of a pixel whose raw log-scale is at the clamp, one storage ulp
        # below, one above, far below; pixel 8: a far-tail pixel (18 scales: the tanh-CDF difference is exactly 0, under the floor)
        for j, v in enumerate((-9.0, storage_ulp(tdt, -9.0, True), storage_ulp(tdt, -9.0, False), -20.0)):
            put(p, 4 + j, 0, x0 - 1.0 / 255.0 + 0.5 * math.exp(-9.0))
            put(p, 4 + j, C, v)
        put(p, 8, 0, x0 + 0.9)
        put(p, 8, C, -3.0)
        inp["x"], inp["params"] = x, p.to(tdt)
        if op == "cf_dgauss_bwd":
            cf = head(True)
            for j, v in enumerate((-9.0, storage_ulp(tdt, -9.0, True), storage_ulp(tdt, -9.0, False), -20.0)):
                put(cf, 4 + j, C, v)
            inp["cf"] = cf.to(tdt)
            inp["g_cfx"] = torch.randn(n, C, h, w, generator=g)
            _cf_directed(case, inp, tdt, put, directed)
    inp["directed"] = directed.view(n, h, w)
    if op.endswith("_bwd") and op != "cf_dgauss_bwd":
        inp["coef"] = (0.013 * (1.0 + torch.arange(n if case.get("coef_stride") else 1))).float()
    return inp


def _cf_decode(raw, C, ar):
    """DGaussNet.sample(h) with return_loc=True (vae.py:352-385, 413-422) on raw head outputs [.., pc]: (pre-clamp means, clamped
    means, scale)."""
    ls = raw[..., C:2 * C].clamp(min=-9.0)
    if ar:
        k = torch.tanh(raw[..., 6:9])
        pre0 = raw[..., 0]
        l0 = pre0.clamp(-1, 1)
        pre1 = raw[..., 1] + k[..., 0] * l0
        l1 = pre1.clamp(-1, 1)
        pre2 = raw[..., 2] + k[..., 1] * l0 + k[..., 2] * l1
        pre = torch.stack([pre0, pre1, pre2], -1)
    else:
        pre = raw[..., :C]
    return pre, pre.clamp(-1, 1), ls.exp()


def _cf_forward(rec, cf, x, C, ar):
    rpre, rloc, rsc = _cf_decode(rec, C, ar)
    cpre, cloc, csc = _cf_decode(cf, C, ar)
    u = (x - rloc) / rsc.clamp(min=1e-12)
    y = cloc + csc * u
    return rpre, cpre, y


def _cf_near(inp, C, ar):
    rpre, cpre, y = _cf_forward(inp["params"].double(), inp["cf"].double(), inp["x"].double(), C, ar)
    near = lambda v: ((v.abs() - 1.0).abs() <= NEAR).any(-1)  # noqa: E731
    return near(rpre) | near(cpre) | near(y)


def _cf_directed(case, inp, tdt, put, directed):
    """Draw again the bulk pixels that came out next to a clamp end (a far-from-everything pixel takes their place), then the
    directed ones: pixels 9..: y outside [-1, 1]; each pre-clamp mean of both heads outside [-1, 1]."""
    C, pc = case.c, T.param_channels(case)
    ar = C == 3 and pc >= 9
    bad = _cf_near(inp, C, ar) & ~directed.view(inp["x"].shape[:3])
    safe = torch.zeros(pc, dtype=torch.float64)
    safe[:C] = 0.25
    safe[C:2 * C] = -1.0
    for k in ("params", "cf"):
        inp[k][bad] = safe.to(tdt)
    inp["x"][bad] = 0.5
    rec, cf, x = inp["params"], inp["cf"], inp["x"]
    px = 9
    for sgn in (-1.0, 1.0):  # y = cloc + csc * u far outside
        put(cf, px, 0, 0.5 * sgn), put(cf, px, C, 0.0), put(rec, px, 0, 0.0), put(rec, px, C, -2.0), put(x, px, 0, sgn * 1.0)
        px += 1
    for t in (rec, cf):
        for ch in range(C):
            for sgn in (-1.0, 1.0):
                put(t, px, ch, 3.5 * sgn)  # (|k| < 1 and |loc| <= 1: the autoregressive terms move it by less than 2)
                px += 1


# =============================================================================================================== helpers
def _chunk_sum(t, chunk):
    """[n, m] -> [n, ceil(m / chunk)] sums of consecutive runs."""
    n, m = t.shape
    nch = -(-m // chunk)
    return F.pad(t, (0, nch * chunk - m)).view(n, nch, chunk).sum(-1)


def _reduced(term, A, chunk, chain, excl=None):
    """A chunk-summed output: per-sample element terms [n, m] -> Out over [n, nch]."""
    o = Out(ref=_chunk_sum(term, chunk), A=_chunk_sum(A, chunk), S=chain * _chunk_sum(term.abs(), chunk), terms=(term, A), storage=False)
    if excl is not None:
        o.loose = _chunk_sum(term.abs() * excl, chunk)
        o.excl = excl
    return o


def _kl(ql, qs, pl, ps):
    term = hvae_ref.gaussian_kl(ql, qs, pl, ps)
    A = 0.5 + ps.abs() + qs.abs() + 0.5 * (qs.exp().pow(2) + (ql - pl).pow(2)) / ps.exp().pow(2)
    return term, A


def _grads(loss, leaves):
    return torch.autograd.grad(loss, leaves, allow_unused=True)


# =============================================================================================================== references
def reference(case, inp, dt=torch.float64):
    """name -> Out for every output of the case.  A, S and the masks are meaningful in float64 only."""
    fn = globals()["_ref_" + case.op]
    return fn(case, {k: (v.to(dt) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in inp.items()}, dt)


def _ref_reparam_kl_fwd(case, i, dt):
    lt = f32(case.get("logt"))
    ql, qs, pl, ps, eps = i["q_loc"], i["q_ls"] + lt, i["p_loc"], i["p_ls"] + lt, i["eps"]
    sq = qs.exp()
    term, A = _kl(ql, qs, pl, ps)
    n = case.n
    out = {"z": Out(ql + sq * eps, ql.abs() + (sq * eps).abs()),
           "kl_part": _reduced(term.reshape(n, -1), A.reshape(n, -1), T.LAT_CHUNK, 8 + 6 + 2)}  # 8 per thread, the 64-lane tree, 4 waves
    if case.get("eps_out"):
        out["eps_out"] = Out(eps, exact=True)
    return out


def _ref_sample_gaussian(case, i, dt):
    sq = (i["q_ls"] + f32(case.get("logt"))).exp()
    return {"z": Out(i["q_loc"] + sq * i["eps"], i["q_loc"].abs() + (sq * i["eps"]).abs())}


def _ref_reparam_kl_bwd(case, i, dt):
    lt = f32(case.get("logt"))
    n, c = case.n, case.c
    leaves = [i[k].clone().requires_grad_(True) for k in ("q_loc", "q_ls", "p_loc", "p_ls")]
    ql, qs, pl, ps = leaves[0], leaves[1] + lt, leaves[2], leaves[3] + lt
    coef = i["coef"][torch.arange(n, device=ql.device) * case.get("coef_stride")].view(n, 1, 1, 1)
    k = coef * (i["chan_scale"].view(1, 1, 1, c) if case.get("cs") else 1.0)
    loss = (k * hvae_ref.gaussian_kl(ql, qs, pl, ps)).sum()
    gz, z = i["gz"], i["z"]
    if case.get("gz"):  # the kernel reads the STORED z: dz / dq_ls = exp(q_ls) eps = z - q_loc
        eps_eff = ((z - ql) / qs.exp()).detach()
        loss = loss + (gz * (ql + qs.exp() * eps_eff)).sum()
    g = _grads(loss, leaves)
    with torch.no_grad():
        e2q, ie2p, d = (2 * qs).exp(), (-2 * ps).exp(), ql.abs() + pl.abs()
        ka = k.abs() * torch.ones_like(ql)
        A = [ka * d * ie2p, ka * (e2q * ie2p + 1.0), ka * d * ie2p, ka * (1.0 + (e2q + d * d) * ie2p)]
        if case.get("gz"):
            A[0] = A[0] + gz.abs()
            A[1] = A[1] + gz.abs() * (z.abs() + ql.abs())
    out = {}
    for j, name in enumerate(("g_q_loc", "g_q_ls", "g_p_loc", "g_p_ls")):
        acc = case.get("acc_q") if j < 2 else case.get("acc_p")
        out[name] = Out(g[j] + (i[name] if acc else 0.0), A[j] + (i[name].abs() if acc else 0.0))
    return out


def _ref_reparam_kl_bwd_rider(case, i, dt):
    out = _ref_reparam_kl_bwd(case, i, dt)
    if case.get("ride_acc"):  # one f32 sum of two stored values
        out["ride_dst"] = Out(i["ride_src"] + i["ride_dst"], i["ride_src"].abs() + i["ride_dst"].abs())
    else:
        out["ride_dst"] = Out(i["ride_src"], exact=True)
    return out


def _ref_mediator_mix(case, i, dt):
    """vae.py:505 (variances weighted by a^2, (1-a)^2) / simple_vae.py:385 (by a, 1-a): u = (z - q_loc) / q_scale,
    out = a q_loc + (1-a) p_loc + sqrt(wq q_scale^2 + wp p_scale^2) [* t] * u."""
    a, t, lv = f32(case.get("alpha")), f32(case.get("t")), case.get("linear_var")
    lt = f32(math.log(t)) if t > 0 else 0.0
    qsc, psc = (i["q_ls"] + lt).exp(), (i["p_ls"] + lt).exp()
    u = (i["z"] - i["q_loc"]) / qsc
    wq, wp = (a, 1.0 - a) if lv else (a * a, (1.0 - a) * (1.0 - a))
    rs = torch.sqrt(wq * qsc * qsc + wp * psc * psc) * (t if t > 0 else 1.0)
    ref = a * i["q_loc"] + (1.0 - a) * i["p_loc"] + rs * u
    A = abs(a) * i["q_loc"].abs() + abs(1.0 - a) * i["p_loc"].abs() + rs * (i["z"].abs() + i["q_loc"].abs()) / qsc
    return {"out": Out(ref, A)}


def _ref_kl_channel_sums(case, i, dt):
    lt = f32(case.get("logt"))
    term, A = _kl(i["q_loc"], i["q_ls"] + lt, i["p_loc"], i["p_ls"] + lt)
    n, c, hw = case.n, case.c, case.h * case.w
    lanes = 256 // c
    chain = -(-hw // lanes) + int(math.log2(lanes))  # a thread's pixels, then the LDS tree over the lanes of a channel
    t, a = term.reshape(n, hw, c), A.reshape(n, hw, c)
    return {"out": Out(t.sum(1), a.sum(1), chain * t.abs().sum(1), terms=(term, A), storage=False)}


def _ref_gaussian_kl_map(case, i, dt):
    term, A = _kl(i["q_loc"], i["q_ls"], i["p_loc"], i["p_ls"])
    return {"out": Out(term, A, storage=False)}


# ----------------------------------------------------------------------------------------------- discretised Gaussian
def _dg_loc(raw, x, C, ar):
    """Training-time means: autoregressive on the TRUE pixels (vae.py:370-377)."""
    loc = raw[..., :C]
    if ar:
        k = torch.tanh(raw[..., 6:9])
        loc = torch.stack([loc[..., 0], loc[..., 1] + k[..., 0] * x[..., 0], loc[..., 2] + k[..., 1] * x[..., 0] + k[..., 2] * x[..., 1]], -1)
    return loc


def _dg_lp(raw, x, C, ar):
    loc, ls = _dg_loc(raw, x, C, ar), raw[..., C:2 * C].clamp(min=hvae_ref.MIN_LOGSCALE)
    flat = lambda t: t.reshape(-1, 1, 1, 1)  # noqa: E731  (every element its own "sample": the oracle's mean is the element)
    return -hvae_ref.dgauss_nll_from_params(flat(loc), flat(ls), flat(x)).reshape(x.shape)


def _dg_cdf_grad(u, sign=-1.0):
    """dg_cdf_grad; sign = +1: its absolute-value computation (1 - t^2 cancels in the tails)."""
    t = torch.tanh(math.sqrt(2.0 / math.pi) * (u + 0.044715 * u ** 3))
    return 0.5 * (1.0 + sign * t * t) * math.sqrt(2.0 / math.pi) * (1.0 + 3.0 * 0.044715 * u * u)


def _dg_explicit(raw, x, C, ar):
    """The pieces of dg_logp / dg_logp_grad, for A and the exclusion mask (float64, no autograd)."""
    loc, lsr = _dg_loc(raw, x, C, ar), raw[..., C:2 * C]
    ls = lsr.clamp(min=-9.0)
    inv, d = (-ls).exp(), x - loc
    up, um = inv * (d + HB8), inv * (d - HB8)
    cp, cm = hvae_ref._tanh_cdf(up), hvae_ref._tanh_cdf(um)
    left, right = x < -0.999, x > 0.999
    sel = torch.where(left, cp, torch.where(right, 1.0 - cm, cp - cm))
    ok = sel >= 1e-12
    den = sel.clamp(min=1e-12)
    # cp = 0.5 (1 + tanh(.)) cancels in the lower tail, so its absolute-value computation is 0.5 (1 + |tanh(.)|), not cp itself
    cpa, cma = torch.maximum(cp, 1.0 - cp), torch.maximum(cm, 1.0 - cm)
    amp = torch.where(left, cpa, torch.where(right, 1.0 + cma, cpa + cma)) / den
    amp = torch.where(ok, amp, torch.zeros_like(amp))  # under the floor the term is the constant -log 1e-12: nothing is amplified
    gp, gm = _dg_cdf_grad(up), _dg_cdf_grad(um)
    dup = torch.where(right | ~ok, torch.zeros_like(gp), gp / den)
    dum = torch.where(left | ~ok, torch.zeros_like(gm), -gm / den)
    dupa = torch.where(right | ~ok, torch.zeros_like(gp), _dg_cdf_grad(up, 1.0) / den)
    duma = torch.where(left | ~ok, torch.zeros_like(gm), _dg_cdf_grad(um, 1.0) / den)
    # first-order effect of the roundings of the CDF's argument inv * (x - loc +- 1/255): loc is a sum for RGB, inv an exponential
    loca = raw[..., :C].abs()
    if ar:
        ka, xa = torch.tanh(raw[..., 6:9]).abs(), x.abs()
        loca = torch.stack([loca[..., 0], loca[..., 1] + ka[..., 0] * xa[..., 0], loca[..., 2] + ka[..., 1] * xa[..., 0] + ka[..., 2] * xa[..., 1]], -1)
    da = inv * (x.abs() + loca + HB8)  # the difference's roundings; the exponential's relative error scales the argument itself
    ua_p, ua_m = da + up.abs() * (1.0 + ls.abs()), da + um.abs() * (1.0 + ls.abs())
    dsum = dup.abs() + dum.abs()
    qf = lambda u: 2.0 * math.sqrt(2.0 / math.pi) * (1.0 + 3.0 * 0.044715 * u * u) + 6.0 * 0.044715 * u.abs() + dsum  # noqa: E731  |d log dup / du| <=
    q_p, q_m = qf(up), qf(um)
    s_lp = dup.abs() * ua_p + dum.abs() * ua_m
    s_loc = dup.abs() * q_p * ua_p + dum.abs() * q_m * ua_m
    s_ls = dup.abs() * ua_p * (1.0 + up.abs() * q_p) + dum.abs() * ua_m * (1.0 + um.abs() * q_m)
    near = ((x.abs() - 0.999).abs() <= NEAR * 0.999) | ((sel - 1e-12).abs() <= NEAR * 1e-12)
    return dict(s_loc=s_loc, s_ls=s_ls, dsum=dsum, lsr=lsr, inv=inv, up=up, um=um, amp=amp, dup=dup, dum=dum, dupa=dupa, duma=duma, near=near, A_lp=amp + torch.log(den).abs() + s_lp)


def _ref_dgauss_nll_fwd(case, i, dt):
    C, ar = case.c, case.c == 3 and T.param_channels(case) >= 9
    raw, x = i["params"], i["x"]
    lp = _dg_lp(raw, x, C, ar)
    e = _dg_explicit(raw.double(), x.double(), C, ar)
    excl = e["near"] & ~i["directed"][..., None]
    n, npx = case.n, case.h * case.w
    # a chunk is LIKE_PIX pixels x C channels, pixel-major: chunk the [n, npx * C] terms by LIKE_PIX * C
    o = _reduced((-lp).reshape(n, npx * C), e["A_lp"].reshape(n, npx * C), T.LIKE_PIX * C, 4 * C + 6 + 2, excl.reshape(n, npx * C).double())
    return {"nll_part": o}


def _ref_dgauss_nll_bwd(case, i, dt):
    C, pc = case.c, T.param_channels(case)
    ar = C == 3 and pc >= 9
    n = case.n
    raw, x = i["params"].clone().requires_grad_(True), i["x"]
    coef = i["coef"][torch.arange(n, device=x.device) * case.get("coef_stride")].view(n, 1, 1, 1)
    g, = _grads((coef * -_dg_lp(raw, x, C, ar)).sum(), [raw])
    e = _dg_explicit(i["params"].double(), x.double(), C, ar)
    ca = coef.abs().double()
    A = torch.zeros(raw.shape, dtype=torch.float64, device=x.device)
    # (the rounding of the common denominator multiplies dup + dum, not |dup| + |dum|)
    Al = ca * e["inv"] * (e["dupa"] + e["duma"] + (e["dup"] + e["dum"]).abs() * e["amp"] + e["s_loc"])
    A[..., :C] = Al
    wsum = (e["dup"] * e["up"] + e["dum"] * e["um"]).abs()
    A[..., C:2 * C] = torch.where(e["lsr"] >= -9.0, ca * ((e["dupa"] * e["up"]).abs() + (e["duma"] * e["um"]).abs() + wsum * e["amp"]
                                                          + e["s_ls"]), 0.0 * Al)
    if ar:
        k2 = 1.0 + torch.tanh(i["params"].double()[..., 6:9]) ** 2
        xa = x.double().abs()
        A[..., 6:9] = torch.stack([Al[..., 1] * xa[..., 0], Al[..., 2] * xa[..., 0], Al[..., 2] * xa[..., 1]], -1) * k2
    excl = (e["near"].any(-1) & ~i["directed"])[..., None].expand_as(A)
    return {"g": Out(g, A, excl=excl)}


def _identity_heads(C, pc, dt, dev):
    eye = torch.eye(pc, dtype=dt, device=dev).view(pc, pc, 1, 1)
    sd = {"likelihood.x_loc.weight": eye[:C], "likelihood.x_loc.bias": torch.zeros(C, dtype=dt, device=dev),
          "likelihood.x_logscale.weight": eye[C:2 * C], "likelihood.x_logscale.bias": torch.zeros(C, dtype=dt, device=dev)}
    if C == 3 and pc >= 9:
        sd["likelihood.channel_coeffs.weight"], sd["likelihood.channel_coeffs.bias"] = eye[6:9], torch.zeros(3, dtype=dt, device=dev)
    return sd


def _dg_params(case, i, dt, with_x):
    """(loc, clamped logscale) NCHW through the oracle's DGaussNet.forward on identity 1x1 heads, and the amplification of loc."""
    C, pc = case.c, T.param_channels(case)
    raw = i["params"]
    h = raw.permute(0, 3, 1, 2)
    xn = i["x"].permute(0, 3, 1, 2) if with_x else None
    loc, ls = hvae_ref.dgauss_params(_identity_heads(C, pc, dt, raw.device), None, h, xn)
    A = raw[..., :C].abs().permute(0, 3, 1, 2).clone()
    if C == 3 and pc >= 9:
        k = torch.tanh(raw[..., 6:9]).abs()
        r, gch = (xn[:, 0].abs(), xn[:, 1].abs()) if with_x else (loc[:, 0].abs(), loc[:, 1].abs())
        A[:, 1] = A[:, 1] + k[..., 0] * r
        A[:, 2] = A[:, 2] + k[..., 1] * r + k[..., 2] * gch
    return loc, ls, A


def _ref_dgauss_params(case, i, dt):
    lt = f32(case.get("logt"))
    loc, ls, A = _dg_params(case, i, dt, bool(case.get("x")))
    return {"loc": Out(loc, A, storage=False), "ls": Out(ls + lt, ls.abs() + abs(lt), storage=False)}


def _ref_dgauss_sample(case, i, dt):
    """rng = null: x = clamp(loc), scale = exp(max(ls, -9) + log t) with t = 1."""
    loc, ls, A = _dg_params(case, i, dt, False)
    return {"x": Out(loc.clamp(-1.0, 1.0), A, storage=False), "scale": Out(ls.exp(), ls.exp() * (1.0 + ls.abs()), storage=False)}


GSCALE = 0.25


def _ref_cf_dgauss_bwd(case, i, dt):
    """dscm.py:52-56 on both heads' decoded (loc, scale): u = (x - rec_loc) / max(rec_scale, 1e-12); cf_x = clamp(cf_loc +
    cf_scale u, -1, 1); the gradient of sum(g_cfx * gscale * cf_x) w.r.t. both raw parameter tensors."""
    C, pc = case.c, T.param_channels(case)
    ar = C == 3 and pc >= 9
    rec, cf = i["params"].clone().requires_grad_(True), i["cf"].clone().requires_grad_(True)
    x, gy = i["x"], i["g_cfx"].permute(0, 2, 3, 1) * f32(GSCALE)
    _, _, y = _cf_forward(rec, cf, x, C, ar)
    g_rec, g_cf = _grads((gy * y.clamp(-1.0, 1.0)).sum(), [rec, cf])
    with torch.no_grad():  # the kernel's chain on absolute values
        r64, c64, x64, gy64 = i["params"].double(), i["cf"].double(), x.double(), gy.double().abs()
        (rpre, rloc, rsc), (cpre, cloc, csc) = _cf_decode(r64, C, ar), _cf_decode(c64, C, ar)
        rs = rsc.clamp(min=1e-12)
        ua = (x64.abs() + rloc.abs()) / rs
        y64 = cloc + csc * ((x64 - rloc) / rs)
        gya = gy64 * ((y64 >= -1) & (y64 <= 1))
        inn = lambda v: ((v >= -1) & (v <= 1)).double()  # noqa: E731

        def back(raw, pre, loc, sc, Aloc, Asc):
            A = torch.zeros_like(raw)
            if ar:
                k = torch.tanh(raw[..., 6:9]).abs()
                gb = Aloc[..., 2] * inn(pre[..., 2])
                gg = (Aloc[..., 1] + gb * k[..., 2]) * inn(pre[..., 1])
                A[..., 2], A[..., 1] = gb, gg
                A[..., 0] = (Aloc[..., 0] + gb * k[..., 1] + gg * k[..., 0]) * inn(pre[..., 0])
                la0 = raw[..., 0].abs().clamp(max=1.0)  # |loc| as computed on absolute values: pre1 = raw1 + k0 loc0 can cancel
                la1 = (raw[..., 1].abs() + k[..., 0] * la0).clamp(max=1.0)
                A[..., 6:9] = torch.stack([gg * la0, gb * la0, gb * la1], -1) * (1.0 + k * k)
            else:
                A[..., :C] = Aloc * inn(pre)
            A[..., C:2 * C] = Asc * sc * (raw[..., C:2 * C] >= -9.0) * (1.0 + raw[..., C:2 * C].abs())
            return A

        gu = gya * csc
        A_rec = back(r64, rpre, rloc, rsc, gu / rs, gu * ua / rs * (rsc >= 1e-12))
        A_cf = back(c64, cpre, cloc, csc, gya, gya * ua)
        near = lambda v: ((v.abs() - 1.0).abs() <= NEAR).any(-1)  # noqa: E731
        excl = ((near(rpre) | near(cpre) | near(y64)) & ~i["directed"])[..., None]
    return {"g": Out(g_rec, A_rec, excl=excl.expand_as(A_rec)), "g_cf": Out(g_cf, A_cf, excl=excl.expand_as(A_cf))}


# ----------------------------------------------------------------------------------------------- logit-space Gaussian
def gauss_terms(raw, x, u, C):
    """simple_vae.py:215-229 with the f32 clamp of torch's SigmoidTransform.inv (what gs_target uses in every dtype): per-element
    -log N(logit(v); loc, exp(max(ls, -9)))."""
    loc, ls = raw[..., :C], raw[..., C:2 * C].clamp(min=simple_ref.EPS)
    v = (((x + 1.0) * 127.5 + u) / 256.0).clamp(min=F32_TINY, max=1.0 - F32_EPS)
    tgt = v.log() - (-v).log1p()
    d = (tgt - loc) / ls.exp()
    return 0.5 * d * d + ls + 0.5 * math.log(2 * math.pi), v, tgt, d, ls


def _gs_A(raw, x, u, C):
    term, v, tgt, d, ls = gauss_terms(raw, x, u, C)
    va = ((x.abs() + 1.0) * 127.5 + u.abs()) / 256.0
    vraw = ((x + 1.0) * 127.5 + u) / 256.0
    clamped = (vraw <= F32_TINY) | (vraw >= 1.0 - F32_EPS)  # on an active clamp the target is a constant: v's roundings do not reach it
    A_tgt = v.log().abs() + (-v).log1p().abs() + torch.where(clamped, torch.zeros_like(v), va * (1.0 / v + 1.0 / (1.0 - v)))
    inv = (-ls).exp()
    A_d = (A_tgt + raw[..., :C].abs()) * inv + d.abs() * (1.0 + ls.abs())  # (the exponential's relative error scales d itself)
    return term, d, inv, A_d, d.abs() * A_d + 0.5 * d * d + ls.abs() + 0.9189385332046727


def _ref_gauss_nll_fwd(case, i, dt):
    C, n, npx = case.c, case.n, case.h * case.w
    term = gauss_terms(i["params"], i["x"], i["u"], C)[0]
    A = _gs_A(i["params"].double(), i["x"].double(), i["u"].double(), C)[4]
    return {"nll_part": _reduced(term.reshape(n, npx * C), A.reshape(n, npx * C), T.LIKE_PIX * C, 4 * C + 6 + 2)}


def _ref_gauss_nll_bwd(case, i, dt):
    C, n = case.c, case.n
    raw = i["params"].clone().requires_grad_(True)
    coef = i["coef"][torch.arange(n, device=raw.device) * case.get("coef_stride")].view(n, 1, 1, 1)
    g, = _grads((coef * gauss_terms(raw, i["x"], i["u"], C)[0]).sum(), [raw])
    _, d, inv, A_d, _ = _gs_A(i["params"].double(), i["x"].double(), i["u"].double(), C)
    ca = coef.abs().double()
    A = torch.cat([ca * inv * A_d, torch.where(i["params"].double()[..., C:2 * C] >= -9.0, ca * (1.0 + d * d + 2.0 * d.abs() * A_d), 0.0 * d)], -1)
    return {"g": Out(g, A)}


# ----------------------------------------------------------------------------------------------- mixture of logistics
def _dm_explicit(l, x, hb, logc):
    """dm_logprob / dm_pixel piece by piece (float64, no autograd): amplifications of the pixel's log-probability and of its 100
    gradients, and the pixels with a component next to the delta = 1e-5 switch."""
    logits, means, lsr, co = dmol_ref._unpack(l)
    ls, k = lsr.clamp(min=-7.0), torch.tanh(co)
    xe = x.unsqueeze(-1).expand(*x.shape, 10)
    mu = torch.stack([means[..., 0, :], means[..., 1, :] + k[..., 0, :] * xe[..., 0, :],
                      means[..., 2, :] + k[..., 1, :] * xe[..., 0, :] + k[..., 2, :] * xe[..., 1, :]], dim=3)
    inv, d = (-ls).exp(), xe - mu
    up, um, mid = inv * (d + hb), inv * (d - hb), inv * d
    cp, cm = torch.sigmoid(up), torch.sigmoid(um)
    de = cp - cm
    left, right = xe < -0.999, xe > 0.999
    inter = ~left & ~right & (de > 1e-5)
    fb = ~left & ~right & ~inter
    den = de.clamp(min=1e-12)
    z = torch.zeros_like(de)
    lp = torch.where(left, up - F.softplus(up), torch.where(right, -F.softplus(um), torch.where(inter, den.log(), mid - ls - 2 * F.softplus(mid) - logc)))
    amp = torch.where(inter, (cp + cm) / den, torch.ones_like(de))
    A_lp = torch.where(left, up.abs() + F.softplus(up), torch.where(right, F.softplus(um), torch.where(
        inter, amp + lp.abs(), mid.abs() + ls.abs() + 2 * F.softplus(mid) + logc)))
    dup = torch.where(left, 1 - cp, torch.where(inter, cp * (1 - cp) / den, z))
    dum = torch.where(right, -cm, torch.where(inter, -cm * (1 - cm) / den, z))
    dmid = torch.where(fb, 1 - 2 * torch.sigmoid(mid), z)
    lsm = dmol_ref._log_softmax(logits)
    lse = (logits - lsm)[..., :1]
    S = lp.sum(3) + lsm
    out = torch.logsumexp(S, -1)
    wm, pim = (S - out[..., None]).exp(), lsm.exp()
    A_S = A_lp.sum(3) + logits.abs() + lse.abs()
    A_out = (wm * A_S).sum(-1) + out.abs()
    R = A_S + A_out[..., None]
    dmean = -(dup + dum + dmid) * inv
    # 1 - cp, 1 - cm and 1 - 2 sigmoid(mid) cancel: on absolute values they are 1 + cp, 1 + cm, 1 + 2 sigmoid(mid)
    dupa = torch.where(left, 1 + cp, torch.where(inter, cp * (1 + cp) / den, z))
    duma = torch.where(right, cm, torch.where(inter, cm * (1 + cm) / den, z))
    dmida = torch.where(fb, 1 + 2 * torch.sigmoid(mid), z)
    A_dmean = (dupa + duma + dmida + (dup + dum).abs() * amp) * inv
    passf = torch.where(lsr > -7.0, torch.ones_like(de), torch.where(lsr == -7.0, 0.5 * torch.ones_like(de), z))
    dls = passf * (-(dup * up + dum * um + dmid * mid) - fb.double())
    A_dls = passf * ((dupa * up).abs() + (duma * um).abs() + (dmida * mid).abs() + fb.double() + (dup * up + dum * um).abs() * amp)
    w3, R3 = wm.unsqueeze(3), R.unsqueeze(3)
    A_mean = w3 * (R3 * dmean.abs() + A_dmean)
    A_ls = w3 * (R3 * dls.abs() + A_dls)
    xa = x.abs()
    A_co = torch.stack([A_mean[..., 1, :] * xa[..., 0, None], A_mean[..., 2, :] * xa[..., 0, None], A_mean[..., 2, :] * xa[..., 1, None]], 3) * (1 + k * k)
    A_g = torch.cat([wm * R + pim * (logits.abs() + lse.abs()) + wm + pim, torch.cat([A_mean, A_ls, A_co], -1).reshape(*x.shape[:-1], 90)], -1)
    # next to the delta switch: within the relative NEAR, or within reach of delta's own f32 rounding, 2^-24 (cp + cm) each way (the
    # tables' draws keep every delta above 5e-5; dmol_lowbit.pt has one pixel whose f32 and f64 deltas straddle 1e-5)
    reach = torch.maximum(torch.full_like(de, NEAR * 1e-5), 2.0 * U32 * (cp + cm))
    near = (~left & ~right & ((de - 1e-5).abs() <= reach)).any(-1).any(-1) | ((x.abs() - 0.999).abs() <= NEAR * 0.999).any(-1)
    return out, A_out, A_g, near


def _dm_logp(l, x, low):
    """log p per pixel through the oracle: every pixel its own 1 x 1 "image" (the oracle returns -log p / 3 of it)."""
    return -3.0 * dmol_ref.dmol_nll(x.reshape(-1, 1, 1, 3), l.reshape(-1, 1, 1, 100), low_bit=low).reshape(x.shape[:-1])


def _ref_dmol_nll_fwd(case, i, dt):
    low = bool(case.get("low_bit"))
    n, npx = case.n, case.h * case.w
    lp = _dm_logp(i["params"], i["x"], low)
    _, A_out, _, near = _dm_explicit(i["params"].double(), i["x"].double(), HB5 if low else HB8, LOGC5 if low else LOGC8)
    excl = near & ~i["directed"]
    return {"nll_part": _reduced((-lp).reshape(n, npx), A_out.reshape(n, npx), T.LIKE_PIX, 4 + 6 + 2, excl.reshape(n, npx).double())}


def _ref_dmol_nll_bwd(case, i, dt):
    low = bool(case.get("low_bit"))
    n = case.n
    l = i["params"].clone().requires_grad_(True)
    coef = i["coef"][torch.arange(n, device=l.device) * case.get("coef_stride")].view(n, 1, 1)
    g, = _grads((coef * -_dm_logp(l, i["x"], low)).sum(), [l])
    _, _, A_g, near = _dm_explicit(i["params"].double(), i["x"].double(), HB5 if low else HB8, LOGC5 if low else LOGC8)
    A = coef.abs().double()[..., None] * A_g
    return {"g": Out(g, A, excl=(near & ~i["directed"])[..., None].expand_as(A))}


# ----------------------------------------------------------------------------------------------------------- ELBO
NLL_DIV, KL_DIV = 192.0, 3.0


def _ref_elbo_finalize(case, i, dt):
    """out3 = (nll + beta kl, nll, kl): per-sample partial sums / div, batch mean.  Chains: a lane's ceil(count / 64) partials, the
    64-lane tree, the division, the n-term serial sum, the mean."""
    n, nc, kc = case.n, case.get("nll_count"), case.get("kl_count")
    beta = f32(i["beta"])
    a_t, k_t = i["nll_part"].view(n, nc) / NLL_DIV / n, i["kl_part"].view(n, kc) / KL_DIV / n
    a, k = a_t.sum(), k_t.sum()
    ta = (-(-nc // 64) + 6 + n + 2) * a_t.abs().sum()
    tk = (-(-kc // 64) + 6 + n + 2) * k_t.abs().sum()
    ref = torch.stack([a + beta * k, a, k])
    S = torch.stack([ta + abs(beta) * tk + 2 * (a.abs() + abs(beta) * k.abs()), ta, tk])
    return {"out3": Out(ref, torch.zeros_like(S), S, storage=False)}


def _ref_elbo_finalize_fb(case, i, dt):
    """vae.py:443-457: kl = sum_j max(fb, mean_b S[b][j]) / kl_div; chan_mask = 1 above the threshold, 0 below, 1/2 on a tie.
    Chains: nll_count serial, the division, n serial, the mean; a column's n serial + the division, a thread's ceil(ncol / 256)
    columns, the 256 serial, the division."""
    n, nc, ncol = case.n, case.get("nll_count"), case.get("ncol")
    beta, fbits = f32(i["beta"]), f32(FREE_BITS)
    a_t = i["nll_part"].view(n, nc) / NLL_DIV / n
    a = a_t.sum()
    m = i["kl_bc"].view(n, ncol).mean(0)
    k = torch.clamp(m, min=fbits).sum() / KL_DIV
    ta = (nc + n + 2) * a_t.abs().sum()
    tk = (n + 1 + -(-ncol // 256) + 256 + 1) * torch.clamp(i["kl_bc"].view(n, ncol).abs().mean(0), min=fbits).sum() / KL_DIV
    ref = torch.stack([a + beta * k, a, k])
    S = torch.stack([ta + abs(beta) * tk + 2 * (a.abs() + abs(beta) * k.abs()), ta, tk])
    mask = torch.where(m > fbits, 1.0, torch.where(m == fbits, 0.5, 0.0)).to(m.dtype)
    near = (m - fbits).abs() <= NEAR * fbits
    return {"out3": Out(ref, torch.zeros_like(S), S, storage=False),
            "chan_mask": Out(mask, exact=True, storage=False, excl=near & (m != fbits))}


# ============================================================================================================ measuring K
def measure_k(case, tdt=torch.float32):
    """Largest |f32 evaluation - f64 reference| / (2^-24 A) over the compared elements of the case's outputs (element results, and
    the element terms of the reduced ones)."""
    inp = make_inputs(case, tdt)
    r64, r32 = reference(case, inp, torch.float64), reference(case, inp, torch.float32)
    worst = 0.0
    for name, o in r64.items():
        if o.exact or (o.A is None):
            continue
        if o.terms is not None:
            v64, A, v32 = o.terms[0], o.terms[1], r32[name].terms[0]
            ex = o.excl
        elif o.S is None:
            v64, A, v32, ex = o.ref, o.A, r32[name].ref, o.excl
        else:
            continue
        err = (v32.double() - v64).abs()
        keep = torch.ones_like(err, dtype=torch.bool) if ex is None else ~ex.bool().reshape(err.shape)
        ratio = torch.where(err == 0, torch.zeros_like(err), err / (U32 * A.reshape(err.shape)))
        ratio = ratio[keep]
        if ratio.numel():
            worst = max(worst, float(ratio.max()))
    return worst


def excluded_fraction(case, tdt):
    inp = make_inputs(case, tdt)
    worst = 0.0
    for o in reference(case, inp).values():
        if o.excl is not None:
            worst = max(worst, float(o.excl.double().mean()))
        assert torch.isfinite(o.ref).all()
    return worst
