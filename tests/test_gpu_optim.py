"""The optimiser tail (csrc/optim.hip: sumsq_partial -> clip_decide -> adamw_ema -> step_commit) driven through step_tail.StepTail
(what the training steps run; test_count_zero and the direct side of test_step_tail_issues_the_direct_sequence call _lib) on flat f32
buffers with a hand-set state vector, against an f64 restatement built from oracle/train_ref (linear_warmup, clip_coef, ema_decay
and the AdamW lines of RefTrainer.apply_grads), and over a 120-step sequence against RefTrainer.apply_grads itself.

State layout (optim.hip): [0] sum of squares [1] norm [2] clip coefficient [3] skip flag [4] skipped steps [5] successful steps
[6] skips for a non-finite norm.  [7] is not the kernels': it must stay as set.

Bound of the element-wise comparison (u = 2^-24), with the hyper-parameters rounded to f32 on both sides and the kernel's own clip
coefficient (itself checked against the f64 norm to 1e-5) fed to the reference:
  m: 8u (|m0| + |g c|)     v: 8u v     update = lr / (1 - b1^t) * m / denom: 128u |update| + lr / (1 - b1^t) * tol(m) / denom
  p: 8u (|p0| + |update|) + tol(update)     ema: tol(p) + 8u (|ema0| + |p|) when averaging
The 128u covers the f32 bias corrections: 1 - powf(0.9, t) loses at most log2(10) bits to cancellation, and lr t0 / warmup,
1 - lr wd and the square root add a few roundings each."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

from oracle import train_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EMA_AFTER = 100  # what TrainStep passes (the reference EMA's update_after_step)
WARMUP = 50
NAN = float("nan")


def f32(v):
    return float(np.float32(v))


def _hp(clip=1e3, skip=1e5, warmup=WARMUP):
    return types.SimpleNamespace(lr=f32(1e-3), betas=[f32(0.9), f32(0.9)], wd=f32(0.01), ema_rate=f32(0.999), lr_warmup_steps=warmup,
                                 grad_clip=clip, grad_skip=skip)


@pytest.fixture(scope="module")
def lib():
    from causal_gen_amd import _lib

    return _lib.require_gpu()


def run_tail(lib, b, state, hp, nblk=1024, out3=None, ranges=None, ema=True, ema_only=()):
    """One optimiser step through step_tail.StepTail, the code the three training steps run, on the caller's moments and state
    vector.  b: dict of flat f32 cuda buffers p, g, m, v, ema."""
    from causal_gen_amd.step_tail import HyperParams, StepTail

    tail = StepTail(lib, 0, "cuda", nblk)
    tail.m, tail.v, tail.state = b["m"], b["v"], state
    tail.partial.fill_(NAN)
    tail.run(HyperParams(hp.lr, (hp.betas[0], hp.betas[1]), 1e-8, hp.wd, float(hp.grad_clip), float(hp.grad_skip), hp.lr_warmup_steps,
                         hp.ema_rate, EMA_AFTER),
             b["p"], b["g"], b["ema"] if ema else None, out3, torch.cuda.current_stream().cuda_stream, ranges=ranges, ema_only=ema_only)
    torch.cuda.synchronize()


def test_step_tail_issues_the_direct_sequence(lib):
    """StepTail.run against the same launches issued here through _lib on cloned buffers, one element past a 256-thread block:
    two ranges with a gap and an EMA-only region.  Every buffer the tail writes is bit-identical, the gap is untouched."""
    from causal_gen_amd import _lib

    count, ranges, nb = 257, [(0, 100), (130, 257)], 33
    b0 = _bufs(count, 41, 5.0)
    hp = _hp(clip=0.5 * float(b0["g"].double().norm()))  # clipped, not skipped
    gen = torch.Generator(device="cuda").manual_seed(42)
    pb0, eb0 = torch.randn(nb, generator=gen, device="cuda"), torch.randn(nb, generator=gen, device="cuda")
    out3 = torch.tensor([1.0, 2.0, 3.0], device="cuda")

    b, state, pb, eb = {k: v.clone() for k, v in b0.items()}, _state(103), pb0.clone(), eb0.clone()
    run_tail(lib, b, state, hp, out3=out3, ranges=ranges, ema_only=[(pb.data_ptr(), eb.data_ptr(), nb)])

    d, dstate, dpb, deb = {k: v.clone() for k, v in b0.items()}, _state(103), pb0.clone(), eb0.clone()
    st = torch.cuda.current_stream().cuda_stream
    partial, zero = torch.full((1024,), NAN, device="cuda"), torch.zeros(3, nb, device="cuda")

    def adamw(p, g, m, v, e, n, lr, wd):
        q = _lib.AdamwArgs()
        q.p, q.g, q.m, q.v, q.ema, q.count = p, g, m, v, e, n
        q.lr, q.beta1, q.beta2, q.eps, q.wd = lr, hp.betas[0], hp.betas[1], 1e-8, wd
        q.ema_beta, q.warmup_steps, q.ema_update_after, q.state_dev = hp.ema_rate, hp.lr_warmup_steps, EMA_AFTER, dstate.data_ptr()
        lib.adamw_ema(C.byref(q), st)

    lib.sumsq_partial(d["g"].data_ptr(), count, partial.data_ptr(), 1024, st)
    lib.clip_decide(partial.data_ptr(), 1024, out3.data_ptr(), float(hp.grad_clip), float(hp.grad_skip), dstate.data_ptr(), st)
    for lo, hi in ranges:
        adamw(*(d[k].data_ptr() + 4 * lo for k in ("p", "g", "m", "v", "ema")), hi - lo, hp.lr, hp.wd)
    adamw(dpb.data_ptr(), zero[0].data_ptr(), zero[1].data_ptr(), zero[2].data_ptr(), deb.data_ptr(), nb, 0.0, 0.0)
    lib.step_commit(dstate.data_ptr(), st)
    torch.cuda.synchronize()

    for k in ("p", "m", "v", "ema"):
        assert torch.equal(_bits(b[k]), _bits(d[k])), k
        assert torch.equal(_bits(b[k][100:130]), _bits(b0[k][100:130])), k  # the gap
        assert not torch.equal(_bits(b[k][:100]), _bits(b0[k][:100])) and not torch.equal(_bits(b[k][130:]), _bits(b0[k][130:])), k
    assert torch.equal(_bits(state), _bits(dstate)) and float(state[5]) == 104.0 and float(state[3]) == 0.0 and float(state[2]) < 1.0
    assert torch.equal(_bits(eb), _bits(deb)) and not torch.equal(_bits(eb), _bits(eb0))  # the statistics' EMA moved ...
    assert torch.equal(_bits(pb), _bits(dpb)) and torch.equal(_bits(pb), _bits(pb0))  # ... the statistics did not (lr = wd = 0, g = 0)
    assert not zero.any()


def ref_update(b0, t0, c, hp):
    """f64 AdamW + EMA of RefTrainer.apply_grads at clip coefficient c after t0 successful steps, with the bound above."""
    p0, g, m0, v0, e0 = (b0[k].double() for k in ("p", "g", "m", "v", "ema"))
    lr = hp.lr * train_ref.linear_warmup(hp.lr_warmup_steps)(t0)
    b1, b2 = hp.betas
    t = t0 + 1
    gc = g * c
    m = m0 + (gc - m0) * (1 - b1)  # (m.lerp_(g, 1 - b1))
    v = v0 * b2 + (1 - b2) * gc * gc
    denom = v.sqrt() / math.sqrt(1 - b2 ** t) + 1e-8
    step = lr / (1 - b1 ** t)
    upd = step * m / denom
    p = p0 * (1 - lr * hp.wd) - upd
    d = train_ref.ema_decay(t0, hp.ema_rate, EMA_AFTER)
    ema = p.clone() if d is None else e0 - (e0 - p) * (1.0 - d)
    tol_m = 8 * U * (m0.abs() + gc.abs())
    tol_upd = 128 * U * upd.abs() + step * tol_m / denom
    tol_p = 8 * U * (p0.abs() + upd.abs()) + tol_upd
    tol_e = tol_p if d is None else tol_p + 8 * U * (e0.abs() + p.abs())
    return {"p": (p, tol_p), "m": (m, tol_m), "v": (v, 8 * U * v), "ema": (ema, tol_e)}


def _bufs(count, seed, gscale, p_scale=0.5):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda s: torch.randn(max(count, 1), generator=g, device="cuda")[:count] * s  # noqa: E731
    return {"p": r(p_scale), "g": r(gscale / math.sqrt(max(count, 1))), "m": r(0.01), "v": r(1e-3).abs() / max(count, 1),
            "ema": r(p_scale)}


def _state(t0, skipped=3.0, nonfinite=2.0):
    return torch.tensor([NAN, NAN, NAN, NAN, skipped, float(t0), nonfinite, 1234.5], device="cuda")


def _bits(t):
    return t.view(torch.int32)


COUNTS = (1, 255, 257, 1024 * 256 + 3, 4096 * 256 + 13)
T0S = (0, 1, WARMUP - 1, WARMUP, WARMUP + 1, 100, 101, 102, 103, 5000, 10 ** 6)
CASES = [(257, 1024, t0, clip) for t0 in T0S for clip in (True, False)]
CASES += [(n, nblk, 103, True) for n in COUNTS for nblk in (1, 1024) if (n, nblk) != (257, 1024)]
CASES += [(n, 1024, t0, False) for n in COUNTS[3:] for t0 in (0, 102, 5000, 10 ** 6)]


@pytest.mark.parametrize("count,nblk,t0,clip", CASES, ids=[f"n{a}-nblk{b}-t{c}-clip{'on' if d else 'off'}" for a, b, c, d in CASES])
def test_step_matches_f64(lib, count, nblk, t0, clip):
    b0 = _bufs(count, count * 31 + t0 % 1000 + nblk, 5.0)
    ss = float((b0["g"].double() ** 2).sum())
    norm = math.sqrt(ss)
    hp = _hp(clip=0.5 * norm if clip else 1e3 * norm, skip=1e5 * norm)  # never skipped
    runs = []
    for _ in range(2):  # two runs from the same inputs: bit-identical
        b = {k: v.clone() for k, v in b0.items()}
        state = _state(t0)
        run_tail(lib, b, state, hp, nblk=nblk)
        runs.append((b, state))
    (b, state), (b2, state2) = runs
    assert torch.equal(_bits(state), _bits(state2)) and all(torch.equal(_bits(b[k]), _bits(b2[k])) for k in b)
    s = state.cpu().double().tolist()
    assert abs(s[0] - ss) <= 1e-5 * ss and abs(s[1] - norm) <= 1e-5 * norm, (s[:2], ss, norm)
    cref = train_ref.clip_coef(norm, hp.grad_clip)
    assert (cref < 1.0) == clip
    assert abs(s[2] - cref) <= 1e-5 * cref, (s[2], cref)
    if not clip:
        assert s[2] == 1.0
    assert s[3:] == [0.0, 3.0, t0 + 1.0, 2.0, 1234.5]
    ref = ref_update(b0, t0, s[2], hp)
    for k, (want, tol) in ref.items():
        err = (b[k].double() - want).abs()
        assert bool((err <= tol).all()), (k, float((err / tol.clamp_min(1e-300)).max()), b[k][:4].tolist(), want[:4].tolist())


SKIPS = [("norm_at_skip", None, 1.0), ("nan_out3_1", 1, 1.0), ("nan_out3_2", 2, 1.0), ("grad_1e20", None, 1e20)]


@pytest.mark.parametrize("count", (255, 4096 * 256 + 13))
@pytest.mark.parametrize("why,nan_at,gmax", SKIPS, ids=[s[0] for s in SKIPS])
def test_skipped_step_touches_nothing(lib, count, why, nan_at, gmax):
    b0 = _bufs(count, 7 + count, 5.0)
    norm = float(b0["g"].double().norm())
    if gmax != 1.0:
        b0["g"][count // 2] = gmax  # g^2 overflows f32: the norm is +inf
    # norm_at_skip: grad_skip equal to the f32 norm the kernel computes (a norm AT the threshold skips, as in the reference)
    hp = _hp(clip=1.0, skip=f32(norm) if why == "norm_at_skip" else 1e5)
    out3 = torch.tensor([1.0, 2.0, 3.0], device="cuda")
    if nan_at is not None:
        out3[nan_at] = NAN
    b = {k: v.clone() for k, v in b0.items()}
    state = _state(102)
    if why == "norm_at_skip":  # (the f32 norm: one step that does not skip, at a threshold far away, reads it)
        probe = _state(102)
        run_tail(lib, {k: v.clone() for k, v in b0.items()}, probe, _hp(clip=1.0), out3=out3)
        hp.grad_skip = float(probe[1])
    run_tail(lib, b, state, hp, out3=out3)
    for k in b:
        assert torch.equal(_bits(b[k]), _bits(b0[k])), k
    s = state.cpu().double().tolist()
    assert s[3] == 1.0 and s[4] == 4.0 and s[5] == 102.0 and s[7] == 1234.5
    assert s[6] == (3.0 if gmax != 1.0 else 2.0), s  # only the non-finite norm counts for the loss-scale back-off
    if gmax != 1.0:
        assert math.isinf(s[0]) and math.isinf(s[1])
    if why == "norm_at_skip":  # (the f64 norm may fall just below the kernel's f32 one: the reference is not asked here)
        return
    # the reference skips too
    tr = train_ref.RefTrainer({"w": b0["p"].double().cpu()}, _hp(clip=1.0, skip=hp.grad_skip))
    tr.opt_steps = 102
    tr.apply_grads({"w": b0["g"].double().cpu()}, float(out3[1]), float(out3[2]))
    assert tr.skipped == 1 and tr.opt_steps == 102


def test_nan_in_out3_0_does_not_skip(lib):
    """out3 = [elbo, nll, kl]: only nll and kl are tested (trainer.py's isnan checks)."""
    b0 = _bufs(255, 3, 5.0)
    b = {k: v.clone() for k, v in b0.items()}
    state = _state(102)
    run_tail(lib, b, state, _hp(), out3=torch.tensor([NAN, 2.0, 3.0], device="cuda"))
    assert float(state[3]) == 0.0 and float(state[5]) == 103.0


@pytest.mark.parametrize("t0", (5, 102))
def test_ema_null(lib, t0):
    hp = _hp()
    b0 = _bufs(1000, 11, 5.0)
    b = {k: v.clone() for k, v in b0.items()}
    state = _state(t0)
    run_tail(lib, b, state, hp, ema=False)
    assert torch.equal(_bits(b["ema"]), _bits(b0["ema"]))
    ref = ref_update(b0, t0, float(state[2]), hp)
    for k in ("p", "m", "v"):
        want, tol = ref[k]
        assert bool(((b[k].double() - want).abs() <= tol).all()), k


def test_count_zero(lib):
    """No parameters: adamw_ema launches nothing; the norm is 0, the step is not skipped and counts."""
    from causal_gen_amd import _lib

    b = {k: torch.full((16,), 7.0, device="cuda") for k in ("p", "g", "m", "v", "ema")}
    st = torch.cuda.current_stream().cuda_stream
    state = _state(4)
    before = {k: v.clone() for k, v in b.items()}
    q = _lib.AdamwArgs()
    q.p, q.g, q.m, q.v, q.ema = (b[k].data_ptr() for k in ("p", "g", "m", "v", "ema"))
    q.count, q.lr, q.beta1, q.beta2, q.eps, q.wd, q.ema_beta = 0, 1e-3, 0.9, 0.9, 1e-8, 0.01, 0.999
    q.warmup_steps, q.ema_update_after, q.state_dev = WARMUP, EMA_AFTER, state.data_ptr()
    lib.adamw_ema(C.byref(q), st)
    torch.cuda.synchronize()
    assert torch.equal(_bits(state), _bits(_state(4)))
    partial = torch.full((1024,), NAN, device="cuda")
    lib.sumsq_partial(b["g"].data_ptr(), 0, partial.data_ptr(), 1024, st)
    lib.clip_decide(partial.data_ptr(), 1024, None, 350.0, 500.0, state.data_ptr(), st)
    lib.step_commit(state.data_ptr(), st)
    torch.cuda.synchronize()
    assert state.cpu().tolist() == [0.0, 0.0, 1.0, 0.0, 3.0, 5.0, 2.0, 1234.5]
    for k in b:
        assert torch.equal(_bits(b[k]), _bits(before[k]))


def _sequence(lib, ranges, gap):
    """120 steps on synthetic gradients (clip active on some, one skipped), against RefTrainer.apply_grads after every step."""
    count = 1000
    hp = _hp(clip=4.0, skip=50.0, warmup=WARMUP)
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(count, generator=gen, dtype=torch.float64) * 0.1
    p0 = p0.float().double()
    keys = {"w": slice(0, count)} if gap is None else {"a": slice(0, gap[0]), "gap": slice(*gap), "b": slice(gap[1], count)}
    tr = train_ref.RefTrainer({k: p0[s].clone() for k, s in keys.items()}, hp)
    b = {"p": p0.float().cuda(), "m": torch.zeros(count, device="cuda"), "v": torch.zeros(count, device="cuda"),
         "ema": p0.float().cuda()}
    state = _state(0, skipped=0.0, nonfinite=0.0)
    steps = 0
    for it in range(120):
        scale = 80.0 if it == 60 else (6.0 if it % 3 == 0 else 2.0)  # norm 80: skipped; 6: clipped to 4; 2: as is
        g = torch.randn(count, generator=gen, dtype=torch.float64).float().double()
        if gap is not None:
            g[gap[0]:gap[1]] = 0.0
        g = (g * (scale / g.norm())).float().double()
        b["g"] = g.float().cuda()
        run_tail(lib, b, state, hp, ranges=ranges)
        grads = {k: g[s] for k, s in keys.items() if k != "gap"}
        tr.apply_grads(grads)
        steps += it != 60
        s = state.cpu().tolist()
        assert s[5] == tr.opt_steps == steps and s[4] == tr.skipped
        for name, mine in (("p", b["p"]), ("ema", b["ema"])):
            want = torch.cat([(tr.sd if name == "p" else tr.ema)[k].detach() for k in keys])
            err = (mine.cpu().double() - want).abs()
            assert bool((err <= 2e-6 + 1e-6 * want.abs()).all()), (it, name, float(err.max()))
        for name, mine in (("m", b["m"]), ("v", b["v"])):
            want = torch.cat([(tr.m if name == "m" else tr.v)[k] for k in keys])
            err = (mine.cpu().double() - want).abs()
            assert bool((err <= 1e-5 * (want.abs() + want.abs().max())).all()), (it, name, float(err.max()))
    assert steps == 119 and tr.opt_steps > EMA_AFTER + 3  # the EMA went through 101 (copy), 102 (copy), 103 (2/3) ...


def test_120_steps_match_reference_trainer(lib):
    _sequence(lib, None, None)


def test_120_steps_split_into_ranges(lib):
    """As TrainStep._optim: one adamw_ema launch per used range; an unused gap (zero gradient) stays untouched."""
    _sequence(lib, [(0, 300), (300, 301), (420, 1000)], (301, 420))
