"""The three kernels of csrc/cf_train.hip through _lib, against the f64 restatements of tests/cf_train_ref.py.

Bounds (u = 2^-24), derived as tests/test_gpu_optim.py derives its own, with every input rounded to f32 on both sides:
  cgen_nonfinite_partial   exact (integer counts)
  cgen_cf_lagrange         8u x the sum of the magnitudes of the terms that form a value: c = eps - elbo is one rounding of
                           |eps| + |elbo|, w = lmbda - damping c two more on |lmbda| + |damping| (|eps| + |elbo|), loss = aux - w c a product
                           and a difference on top; aux_loss multiplies by the f32 1 / B (one rounding of the constant, one of the
                           product); the running sums add one rounding of |sum| + |term|
  cgen_lagrange_step       the one-element bounds of tests/test_gpu_optim.py (m 8u, v 8u, update 128u, p 8u, ema 8u); the clamp
                           max(p, 0) never moves p away from the clamped reference
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import cf_train_ref as R

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


def f32(v):
    return float(np.float32(v))


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def lib():
    from causal_gen_amd import _lib

    return _lib.require_gpu()


def _st():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ cgen_nonfinite_partial
# (n, h, w, c, channel stride): 1, 255, 257 and 70 001 logical elements, dense and with a padded channel stride (70 001 is prime:
# one row of pixels), and 7 x 73 x 137 = 70 007 for a count of that size with all four extents above 1 in the index arithmetic
SHAPES = [(1, 1, 1, 1, 1), (1, 1, 1, 1, 8), (1, 5, 17, 3, 3), (1, 5, 17, 3, 8), (1, 1, 257, 1, 1), (1, 257, 1, 1, 4), (1, 1, 70001, 1, 1),
          (1, 70001, 1, 1, 4), (7, 73, 137, 1, 1), (7, 73, 137, 1, 2)]


def _plant(count, how):
    """flat logical indices that get a non-finite value: at the edges of the 256-element runs a block owns"""
    if how == "none":
        return []
    if how == "one":
        return [count - 1]
    edges = [0, 255, 256, 257, 511, 512, 256 * 3 - 1, 256 * 3, 256 * 64, 256 * 64 - 1, 256 * 65, count - 1, count // 2]
    return sorted({i for i in edges if 0 <= i < count})


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("how", ["none", "one", "several"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_nonfinite_partial_counts_are_exact(lib, shape, how, dtype):
    from causal_gen_amd import _lib

    n, h, w, c, sw = shape
    count = n * h * w * c
    h16 = torch.bfloat16 if lib.h16_is_bf16 else torch.float16
    td = torch.float32 if dtype == "f32" else h16
    g = torch.Generator().manual_seed(count + sw)
    logical = torch.randn(n, h, w, c, generator=g)
    vals = [NAN, INF, -INF]
    flat = logical.reshape(-1)
    for k, i in enumerate(_plant(count, how)):
        flat[i] = vals[k % 3]
    # the padding channels hold NaN: a kernel that walked the memory instead of the view would count them
    mem = torch.full((n, h, w, sw), NAN)
    mem[..., :c] = logical
    dev = mem.to(td).cuda()
    for nblk in (1, 3, 64):
        part = torch.full((nblk + 1,), -7, dtype=torch.int32, device="cuda")
        view = _lib.View(dev.data_ptr(), h * w * sw, w * sw, sw, c, 0)
        lib.nonfinite_partial(_lib.F32 if dtype == "f32" else _lib.F16, n, h, w, view, part.data_ptr(), nblk, _st())
        again = torch.full((nblk + 1,), -7, dtype=torch.int32, device="cuda")
        lib.nonfinite_partial(_lib.F32 if dtype == "f32" else _lib.F16, n, h, w, view, again.data_ptr(), nblk, _st())
        torch.cuda.synchronize()
        want = R.nonfinite_counts(logical.numpy(), nblk)
        assert part[:nblk].cpu().tolist() == want.tolist(), (shape, how, nblk)
        assert int(part[nblk]) == -7 and torch.equal(part, again)
        assert int(want.sum()) == len(_plant(count, how))


# ------------------------------------------------------------------------------------------------ cgen_cf_lagrange
LAG_CASES = {
    "c_pos": dict(out3=(1.25, 1.0, 0.25), aux=37.5, add=None, lmbda=0.8, eps=2.0, damping=10.0, nbad=0),
    "c_neg": dict(out3=(3.5, 3.0, 0.5), aux=12.75, add=None, lmbda=0.8, eps=2.0, damping=10.0, nbad=0),
    "damping_0": dict(out3=(1.7, 1.5, 0.2), aux=5.0, add=1.5, lmbda=0.3, eps=1.841216802597046, damping=0.0, nbad=0),
    "with_addend": dict(out3=(2.25, 2.0, 0.125), aux=101.3, add=-7.7, lmbda=1.9, eps=2.0, damping=100.0, nbad=0),
    "nan_elbo": dict(out3=(NAN, 1.0, 0.25), aux=37.5, add=None, lmbda=0.8, eps=2.0, damping=10.0, nbad=0),
    "inf_aux": dict(out3=(1.25, 1.0, 0.25), aux=INF, add=None, lmbda=0.8, eps=2.0, damping=10.0, nbad=0),
    "nan_aux": dict(out3=(1.25, 1.0, 0.25), aux=NAN, add=None, lmbda=0.8, eps=2.0, damping=10.0, nbad=0),
    "nonfinite_count": dict(out3=(1.25, 1.0, 0.25), aux=37.5, add=None, lmbda=0.8, eps=2.0, damping=10.0, nbad=3),
}
BAD = {"nan_elbo", "inf_aux", "nan_aux", "nonfinite_count"}


@pytest.mark.parametrize("name", list(LAG_CASES))
def test_cf_lagrange_matches_f64(lib, name):
    from causal_gen_amd import _lib

    k = LAG_CASES[name]
    B, beta, dims = 3, f32(1.7), 256.0
    seed_scale = f32(1.0 / (B * dims))
    out3 = torch.tensor(k["out3"], device="cuda")
    aux = torch.tensor([k["aux"]], device="cuda")
    add = None if k["add"] is None else torch.tensor([k["add"]], device="cuda")
    lm = torch.tensor([k["lmbda"]], device="cuda")
    beta_dev = torch.tensor([beta], device="cuda")
    nb = 128
    counts = torch.zeros(nb, dtype=torch.int32, device="cuda")
    if k["nbad"]:
        counts[nb - 1] = k["nbad"]  # the last entry: every count is read
    sums0 = [10.5, 20.25, 3.0, 2.5, 0.5, 4.0, 1.0, 99.0]
    runs = []
    for use_beta_dev in (True, False):
        res, coef, gate = (torch.full((m,), -5.0, device="cuda") for m in (4, 3, 3))
        slot = torch.full((2,), -5.0, device="cuda")
        sums = torch.tensor(sums0, device="cuda")
        q = _lib.CfLagrangeArgs()
        q.out3, q.aux_sum, q.aux_add, q.lmbda = out3.data_ptr(), aux.data_ptr(), None if add is None else add.data_ptr(), lm.data_ptr()
        q.beta_dev, q.beta = (beta_dev.data_ptr(), -1.0) if use_beta_dev else (None, beta)
        q.nonfinite, q.n_nonfinite = counts.data_ptr(), nb
        q.inv_b, q.eps, q.damping, q.seed_scale = 1.0 / B, k["eps"], k["damping"], seed_scale
        q.res, q.coef, q.gsq_slot, q.gate, q.sums = res.data_ptr(), coef.data_ptr(), slot.data_ptr(), gate.data_ptr(), sums.data_ptr()
        lib.cf_lagrange(C.byref(q), _st())
        torch.cuda.synchronize()
        runs.append((res, coef, gate, slot, sums))
    for a, b in zip(*runs):  # beta from the device or from the argument, and a rerun: the same bits
        assert torch.equal(_bits(a), _bits(b))
    res, coef, gate, slot, sums = (t.cpu().double().tolist() for t in runs[0])
    assert slot[1] == -5.0
    o3 = [f32(v) for v in k["out3"]]
    want, bad, new_sums, tol_sums = R.lagrange(o3, f32(k["aux"]), None if k["add"] is None else f32(k["add"]), B, f32(k["lmbda"]), f32(k["eps"]),
                                               f32(k["damping"]), seed_scale, beta, k["nbad"], sums0)
    assert bad == (name in BAD)
    got = {"loss": res[0], "aux_loss": res[1], "g_lmbda": res[2], "w": res[3], "coef0": coef[0], "coef1": coef[1], "coef2": coef[2],
           "gsq": slot[0], "gate0": gate[0], "gate1": gate[1], "gate2": gate[2]}
    for key, (w_, tol) in want.items():
        g_ = got[key]
        print(name, key, g_, w_, tol)
        if math.isnan(w_):
            assert math.isnan(g_), key
        elif math.isinf(w_):
            assert g_ == w_, key
        else:
            assert abs(g_ - w_) <= tol, (key, g_, w_, tol)
    if bad:
        assert math.isnan(gate[1])
        assert sums == [10.5, 20.25, 3.0, 2.5, 0.5, 4.0, 2.0, 99.0]  # the running sums untouched, one more bad step
    else:
        assert gate[1] == o3[1] and sums[5] == 5.0 and sums[6] == 1.0 and sums[7] == 99.0
        for i in range(5):
            assert abs(sums[i] - new_sums[i]) <= tol_sums[i], (i, sums[i], new_sums[i])


def test_bad_gate_makes_clip_decide_drop_the_step(lib):
    """The gate triple of a bad step, handed to cgen_clip_decide as out3, sets the skip flag; a good one does not."""
    for nll, skip in ((NAN, 1.0), (1.0, 0.0)):
        gate = torch.tensor([0.5, nll, 0.25], device="cuda")
        partial = torch.tensor([1.0, 2.0, 0.25], device="cuda")
        state = torch.zeros(8, device="cuda")
        lib.clip_decide(partial.data_ptr(), 3, gate.data_ptr(), 350.0, 500.0, state.data_ptr(), _st())
        torch.cuda.synchronize()
        s = state.cpu().tolist()
        assert s[3] == skip and s[0] == 3.25  # (the extra slot is part of the norm)


# ------------------------------------------------------------------------------------------------ cgen_lagrange_step
HP = dict(lr=f32(1e-2), betas=(f32(0.9), f32(0.9)), eps=f32(1e-8), ema_beta=f32(0.999), ema_after=100)


def _lag_step(lib, lag, g, state, ema=True):
    from causal_gen_amd import _lib

    q = _lib.LagrangeStepArgs()
    p = lag.data_ptr()
    q.lmbda, q.m, q.v, q.ema, q.g, q.state_dev = p, p + 4, p + 8, p + 12 if ema else None, g.data_ptr(), state.data_ptr()
    q.lr, q.beta1, q.beta2, q.eps, q.ema_beta, q.ema_update_after = HP["lr"], HP["betas"][0], HP["betas"][1], HP["eps"], HP["ema_beta"], HP["ema_after"]
    lib.lagrange_step(C.byref(q), _st())


def _state(t0, clip=1.0, skip=0.0):
    return torch.tensor([NAN, NAN, clip, skip, 3.0, float(t0), 2.0, 1234.5], device="cuda")


def test_lagrange_step_120_steps_match_f64(lib):
    """120 steps from a hand-set state vector (the EMA goes through copy, copy, 2/3, ...): each step against f64
    AdamW(maximize=True) + clamp + the reference EMA schedule applied to the state the kernel started the step from."""
    gen = torch.Generator().manual_seed(3)
    lag = torch.tensor([0.1, 0.0, 0.0, 0.1], device="cuda")
    state = _state(0)
    hit_zero = 0
    for it in range(120):
        # the slack c = -g wanders around 0 with a drift towards c > 0 late in the run, so that the multiplier meets the clamp
        gl = f32(float(torch.randn((), generator=gen)) * 0.5 + (0.2 if it < 40 else -0.9))
        clip = f32(0.37) if it % 4 == 0 else 1.0
        g = torch.tensor([gl], device="cuda")
        state[2] = clip
        before = lag.cpu().double().tolist()
        t0 = int(state[5])
        _lag_step(lib, lag, g, state)
        lib.step_commit(state.data_ptr(), _st())
        torch.cuda.synchronize()
        after = lag.cpu().double().tolist()
        want = R.lagrange_step(*before, gl, clip, t0, HP["lr"], HP["betas"], HP["eps"], HP["ema_beta"], HP["ema_after"])
        for i, key in enumerate(("lmbda", "m", "v", "ema")):
            w_, tol = want[key]
            assert abs(after[i] - w_) <= tol, (it, key, after[i], w_, tol)
        assert after[0] >= 0.0
        hit_zero += after[0] == 0.0
    assert int(state[5]) == 120 and hit_zero > 0


@pytest.mark.parametrize("t0", [0, 100, 101, 102, 103, 5000])
def test_lagrange_step_ema_phases(lib, t0):
    lag0 = [0.5, 0.01, 2e-4, 0.7]
    lag = torch.tensor(lag0, device="cuda")
    gl = f32(-0.3)
    _lag_step(lib, lag, torch.tensor([gl], device="cuda"), _state(t0, clip=f32(0.5)))
    torch.cuda.synchronize()
    got = lag.cpu().double().tolist()
    want = R.lagrange_step(*[f32(v) for v in lag0], gl, f32(0.5), t0, HP["lr"], HP["betas"], HP["eps"], HP["ema_beta"], HP["ema_after"])
    for i, key in enumerate(("lmbda", "m", "v", "ema")):
        assert abs(got[i] - want[key][0]) <= want[key][1], (t0, key, got[i], want[key])


def test_lagrange_step_skip_flag_leaves_everything_bit_untouched(lib):
    lag0 = torch.tensor([0.5, 0.01, 2e-4, 0.7], device="cuda")
    lag = lag0.clone()
    state = _state(102, skip=1.0)
    s0 = state.clone()
    _lag_step(lib, lag, torch.tensor([0.3], device="cuda"), state)
    torch.cuda.synchronize()
    assert torch.equal(_bits(lag), _bits(lag0)) and torch.equal(_bits(state), _bits(s0))


def test_lagrange_step_clamps_at_zero_and_the_ema_follows_the_clamped_value(lib):
    """From 0.5 lr with c > 0 (g_lmbda = -c < 0): Adam's first step is lr in size, so the ascent on lmbda lands below zero and is
    clamped to exactly 0; the EMA (copy phase) takes the clamped value, not the one before the clamp."""
    lr = HP["lr"]
    lag = torch.tensor([0.5 * lr, 0.0, 0.0, 0.123], device="cuda")
    _lag_step(lib, lag, torch.tensor([-0.75], device="cuda"), _state(0))
    torch.cuda.synchronize()
    got = lag.cpu().tolist()
    assert got[0] == 0.0 and got[3] == 0.0 and got[1] != 0.0 and got[2] != 0.0
    # ... and in the averaging phase: ema - (ema - 0) (1 - d)
    # (far from t = 1 a first update is lr sqrt(1 - b2) / (1 - b1) ~ 0.32 lr: start below that)
    lag = torch.tensor([0.1 * lr, 0.0, 0.0, 0.5], device="cuda")
    _lag_step(lib, lag, torch.tensor([-0.75], device="cuda"), _state(5000))
    torch.cuda.synchronize()
    got = lag.cpu().double().tolist()
    assert got[0] == 0.0 and abs(got[3] - 0.5 * f32(0.999)) <= 8 * R.U


def test_lagrange_step_without_an_ema(lib):
    lag = torch.tensor([0.5, 0.0, 0.0, 0.123], device="cuda")
    _lag_step(lib, lag, torch.tensor([0.3], device="cuda"), _state(0), ema=False)
    torch.cuda.synchronize()
    assert float(lag[3]) == f32(0.123) and float(lag[0]) != 0.5
