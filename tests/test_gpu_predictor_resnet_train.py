"""ChestPredictorTrainStep on the GPU (causal_gen_amd.predictor_resnet_train, csrc/predictor_resnet_train.inc) against the f64
references of tests/resnet_train_ref.py.

Gradients are compared with the oracle in PINNED mode, as tests/test_gpu_predictor_resnet.py compares the input gradient: every
ReLU mask (times keep / (1 - p) at the Dropout sites) and the max pool's indices are the device's, and the pinning is itself
checked -- wherever the device's decision differs from the oracle's own, the oracle's pre-activation lies within the activation
tolerance of zero.

Tolerances.  Loss: 1e-5 relative.  dx: 1e-4 of its max.  Per parameter tensor: max|err| / max|ref| <= max(1e-5, 4 x e_ref), e_ref
being the same ratio of torch's own f32 CPU run of the pinned oracle on the same inputs (the project's activation rule).  The step:
the element-wise bounds of tests/test_gpu_optim.py's ``ref_update``.

Measured on an MI355X (LABNOTES 31.2 has the worst row of every case's table; the test prints all of them): every tolerance came
out as the 1e-5 floor, the worst parameter gradient is at 5.3e-6 of its tensor's max, the loss at 2.3e-7, dx at 2.7e-6."""
import functools
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import resnet_train_ref as T
from resnet_ref import chest_ref, make_obs, randomise

from oracle import train_ref

pytestmark = pytest.mark.gpu

CASES = {"a": (32, 1), "b": (33, 3), "c": (64, 2), "d": (96, 2)}
BIG = {"e": (192, 2)}  # loss and gradients only
P = 0.2
SEED = 1234  # of the steps' Philox state (torch.manual_seed before construction)


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(b.abs().max()), 1e-30)


def _pred(R, seed=0, std_fixed=0.0):
    from causal_gen_amd.predictor_resnet import ChestPredictor

    return randomise(ChestPredictor(SimpleNamespace(input_channels=1, input_res=R, std_fixed=std_fixed)), 100 + seed)


def _step(pred, **kw):
    from causal_gen_amd.predictor_resnet_train import ChestPredictorTrainStep

    torch.manual_seed(SEED)
    return ChestPredictorTrainStep(pred, **kw)


def _fresh(tag, seed=0, **kw):
    R, B = {**CASES, **BIG, "l": (32, 4)}[tag]
    pred = _pred(R, seed)
    return _step(pred, **kw), pred, make_obs(B, R, 200 + seed)


@functools.lru_cache(maxsize=None)
def _case(tag, p):
    """One device forward + backward and its references, shared by the tests of a case."""
    ts, pred, obs = _fresh(tag, ema=False, use_graph=False, p_dropout=p)
    loss, grads = ts.loss_and_grads(dx=True, **obs)
    acts = [a.cpu() for a in ts.trunk_activations()]
    keeps = [ts.dropout_keep(k).cpu() for k in range(8)]
    terms = ts._last["terms"].clone()
    sd = {k: v.detach().cpu().clone() for k, v in pred.state_dict().items()}
    relu = [(a > 0).double() for a in acts[:17]]
    masks = T.dropout_masks(relu, keeps, p)
    pool_idx = F.max_pool2d(acts[0], 3, 2, 1, return_indices=True)[1]
    pinned = T.loss_and_grads_ref(sd, obs, masks=masks, pool_idx=pool_idx)
    p32 = T.loss_and_grads_ref(sd, obs, masks=masks, pool_idx=pool_idx, dtype=torch.float32)
    e_ref = {n: _rel(p32["grads"][n], pinned["grads"][n]) for n in pinned["grads"]}
    e_act = [_rel(a, b) for a, b in zip(p32["acts"], pinned["acts"])]
    return SimpleNamespace(ts=ts, pred=pred, obs=obs, loss=loss, grads={k: v.cpu() for k, v in grads.items()}, acts=acts, keeps=keeps,
                           terms=terms, sd=sd, relu=relu, masks=masks, pool_idx=pool_idx, pinned=pinned, e_ref=e_ref,
                           act_tol=[max(1e-5, 4 * e) for e in e_act])


def _check_against_the_pinned_oracle(c, tag, p):
    ref = c.pinned
    got, want = float(c.loss), float(ref["loss"])
    print(f"case {tag} p {p}: loss {got:.6f}, oracle {want:.6f}, rel err {abs(got - want) / max(1.0, abs(want)):.3e}")
    assert abs(got - want) <= 1e-5 * max(1.0, abs(want))
    assert set(c.grads) == set(ref["grads"]) | {"x"} and len(ref["grads"]) == 68
    e_x = _rel(c.grads["x"], ref["x"])
    print(f"case {tag} p {p}: dx error {e_x:.3e} of its max {float(ref['x'].abs().max()):.3e}")
    assert c.grads["x"].shape == c.obs["x"].shape and float(ref["x"].abs().max()) > 0 and e_x <= 1e-4
    rows, bad = [], []
    for n, want in ref["grads"].items():
        assert c.grads[n].shape == want.shape and float(want.abs().max()) > 0, n
        err, tol = _rel(c.grads[n], want), max(1e-5, 4 * c.e_ref[n])
        rows.append((err / tol, n, err, c.e_ref[n], tol))
        if not err <= tol:
            bad.append((n, err, tol))
    for ratio, n, err, e32, tol in sorted(rows, reverse=True):
        print(f"case {tag} p {p} {n:44s} device {err:.3e}  torch f32 {e32:.3e}  tolerance {tol:.3e}  ({ratio:.2f} of it)")
    assert not bad, bad


def _check_the_pinning(c, free_pres, free_acts, kept):
    """Wherever the device's ReLU decision differs from the oracle's own at an element Dropout kept, the oracle's pre-activation
    lies within the activation tolerance of zero."""
    flips = 0
    for i, (m, pre, act) in enumerate(zip(c.relu, free_pres, free_acts)):
        diff = (m != (pre > 0).double()) & kept[i]
        n = int(diff.sum())
        flips += n
        if n:
            worst = float(pre[diff].abs().max())
            assert worst <= c.act_tol[i] * float(act.abs().max()), (i, n, worst)
    return flips


# ------------------------------------------------------------------------------------------------ 1. gradients, p_dropout = 0
@pytest.mark.parametrize("tag", sorted(CASES) + sorted(BIG))
def test_loss_and_every_gradient_match_the_pinned_oracle(tag):
    c = _case(tag, 0.0)
    with torch.no_grad():
        free = chest_ref(c.sd, c.obs)
    everything = [torch.ones_like(m, dtype=torch.bool) for m in c.relu]
    flips = _check_the_pinning(c, free["pres"], free["acts"], everything)
    free_idx = F.max_pool2d(free["acts"][0], 3, 2, 1, return_indices=True)[1]
    pool_diff = c.pool_idx != free_idx
    if bool(pool_diff.any()):  # a pinned window may pick another pixel only if the two values tie within tolerance
        stem = free["acts"][0].flatten(2)
        gap = (stem.gather(2, free_idx.flatten(2)) - stem.gather(2, c.pool_idx.flatten(2))).abs()
        assert float(gap.max()) <= c.act_tol[0] * float(stem.abs().max())
    print(f"case {tag}: pinned ReLU disagreements {flips}, pool disagreements {int(pool_diff.sum())}")
    assert all(bool(k.all()) for k in c.keeps)  # p = 0 keeps everything
    _check_against_the_pinned_oracle(c, tag, 0.0)


@pytest.mark.parametrize("tag", sorted(CASES))
def test_without_dropout_the_training_entry_points_leave_the_eval_bits(tag):
    c = _case(tag, 0.0)
    full = {k: v.cuda() for k, v in c.obs.items()}
    B = full["x"].shape[0]
    x = full["x"].clone().requires_grad_(True)
    loss = c.pred.model_anticausal(**dict(full, x=x))
    (gx,) = torch.autograd.grad(loss, x, grad_outputs=torch.full((), 1.0 / B, device="cuda"))
    acts = c.pred.trunk_activations()
    terms = c.pred.nll_terms(**full)
    for i, (got, want) in enumerate(zip(c.acts, acts)):
        assert torch.equal(_bits(got), _bits(want.cpu())), i
    for h, var in enumerate(("sex", "race", "finding", "age")):
        assert torch.equal(_bits(c.terms[:, h]), _bits(terms[var])), var
    assert torch.equal(_bits(c.grads["x"]), _bits(gx.cpu()))


# ------------------------------------------------------------------------------------------------ 2. Dropout
@pytest.mark.parametrize("tag", sorted(CASES))
def test_dropout_masks_scale_and_gradients(tag):
    c, c0 = _case(tag, P), _case(tag, 0.0)
    scale = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(P))  # the kernel's f32 1 / (1 - p)
    for k, site in enumerate(T.A1_SITES):
        keep, a1 = c.keeps[k], c.acts[site]
        assert keep.shape == a1.shape and keep.dtype == torch.bool
        assert bool((a1[~keep] == 0).all()), k
        n, nd = keep.numel(), int((~keep).sum())
        bound = 5 * math.sqrt(n * P * (1 - P))
        print(f"case {tag} block {k}: dropped {nd} of {n} (p N = {P * n:.1f}, bound +- {bound:.1f})")
        assert abs(nd - P * n) <= bound, (k, nd, n)
    keep, a1 = c.keeps[0], c.acts[T.A1_SITES[0]]
    assert torch.equal(_bits(a1[keep]), _bits((c0.acts[T.A1_SITES[0]] * scale)[keep]))  # block 0's input does not see Dropout
    assert not torch.equal(c.keeps[0], c.keeps[1])  # two blocks of one shape
    if keep.shape[0] > 1:
        assert not torch.equal(c.keeps[0][0], c.keeps[0][1])  # two images
    # a device zero at a kept element needs a near-zero pre-activation (the pinned oracle's own, upstream decisions being the device's)
    kept = [torch.ones_like(m, dtype=torch.bool) for m in c.relu]
    for k, site in enumerate(T.A1_SITES):
        kept[site] = c.keeps[k]
    flips = _check_the_pinning(c, c.pinned["pres"], c.pinned["acts"], kept)
    print(f"case {tag} p {P}: pinned ReLU disagreements at kept elements {flips}")
    _check_against_the_pinned_oracle(c, tag, P)


def test_dropout_masks_are_keyed_by_state_block_image_and_element():
    ts, pred, obs = _fresh("b", ema=False, use_graph=False)  # p_dropout = 0.2 by default
    assert ts.p_dropout == P
    ts.loss_and_grads(**obs)
    first = [ts.dropout_keep(k) for k in range(8)]
    ts.loss_and_grads(**obs)
    second = [ts.dropout_keep(k) for k in range(8)]
    assert all(not torch.equal(a, b) for a, b in zip(first, second))  # the state moved on: new masks, eagerly
    again, _, _ = _fresh("b", ema=False, use_graph=False)
    again.loss_and_grads(**obs)
    assert all(torch.equal(a, again.dropout_keep(k)) for k, a in enumerate(first))  # the same seed and offset: the same masks
    alone, _, _ = _fresh("b", ema=False, use_graph=False)
    alone.loss_and_grads(**{k: v[:1] for k, v in obs.items()})
    for k, a in enumerate(first):  # image 0's mask in a batch of 3 is its mask alone
        assert torch.equal(a[:1], alone.dropout_keep(k)), k
    a1 = alone.trunk_activations()[T.A1_SITES[0]]
    assert bool((a1[~alone.dropout_keep(0)] == 0).all())
    # and replayed: the captured sequence holds the state's advance
    cap, _, _ = _fresh("b", ema=False, use_graph=True)
    seen = []
    for i in range(3):
        cap.step(**obs)
        seen.append(cap.dropout_keep(0))
        a1 = cap.trunk_activations()[T.A1_SITES[0]]
        assert bool((a1[~seen[-1]] == 0).all()) and bool((a1[seen[-1]] != 0).any()), i  # the masks the forward really took
    assert len(cap._graphs) == 1 and int(cap._rng[1]) == 3
    assert torch.equal(seen[0], first[0]) and torch.equal(seen[1], second[0])
    assert not torch.equal(seen[1], seen[2]) and not torch.equal(seen[0], seen[2])


# ------------------------------------------------------------------------------------------------ 3. the step
@pytest.mark.parametrize("tag,clip", (("b", 200.0), ("c", 0.05)), ids=("b_clip200", "c_clip_active"))
def test_step_is_the_device_gradient_plus_the_f64_tail(tag, clip):
    hp = SimpleNamespace(lr=f32(1e-3), betas=[f32(0.9), f32(0.999)], wd=f32(0.1), eps=1e-8, ema_rate=f32(0.999), lr_warmup_steps=1,
                         ema_update_after=0)
    kw = dict(lr=hp.lr, wd=hp.wd, betas=hp.betas, ema_rate=hp.ema_rate, lr_warmup_steps=1, ema_update_after=0, grad_clip=clip)
    ts, pred, obs = _fresh(tag, **kw)
    twin, _, _ = _fresh(tag, ema=False, use_graph=False, **kw)
    on, ema = ts._on, ts._ema
    for t0 in range(3):  # (the first step runs at lr = 0: the warm-up; the third is a graph replay)
        b0 = {"p": on.flat_p.clone(), "m": ts.m.clone(), "v": ts.v.clone(), "ema": ema.flat_p.clone()}
        # the twin starts every step from the device's own state: no trajectory drift across a ReLU flip
        sd = ts.state_dict()
        sd.pop("ema_model_state_dict")
        twin.load_state_dict(sd)
        want_loss, want = twin.loss_and_grads(**obs)
        out = ts.step(**obs)
        torch.cuda.synchronize()
        b0["g"] = ts.flat_g.clone()
        for n, o, p in zip(on.names, on.p_off, on.params):
            assert torch.equal(_bits(b0["g"][o:o + p.numel()]), _bits(want[n].reshape(-1))), (t0, n)
        assert torch.equal(_bits(out["loss"]), _bits(want_loss))
        s = ts.state.cpu().double().tolist()
        norm = float(b0["g"].double().norm())
        cref = train_ref.clip_coef(norm, clip)
        assert s[3] == 0.0 and s[4] == 0.0 and s[5] == t0 + 1.0, s
        assert abs(s[1] - norm) <= 1e-5 * norm and abs(s[2] - cref) <= 1e-5 * cref, (s[:3], norm, cref)
        assert (cref < 1.0) == (clip < 1.0) and float(out["grad_norm"]) == s[1]
        ref = T.tail_ref(b0, t0, s[2], hp)
        got = {"p": on.flat_p, "m": ts.m, "v": ts.v, "ema": ema.flat_p}
        for k, (val, tol) in ref.items():
            err = (got[k].double() - val.cuda()).abs()
            assert bool((err <= tol.cuda()).all()), (t0, k, float((err / tol.cuda().clamp_min(1e-300)).max()))
        if t0 == 0:
            assert torch.equal(on.flat_p, b0["p"])  # lr = 0
        else:
            assert not torch.equal(on.flat_p, b0["p"])
    assert ts.stats()["opt_steps"] == 3 and len(ts._graphs) == 1


def test_a_nan_in_the_image_drops_the_step():
    ts, pred, obs = _fresh("a", lr=1e-3, ema_update_after=0)
    ts.step(**obs)
    ts.step(**obs)
    before = {"p": ts._on.flat_p.clone(), "ema": ts._ema.flat_p.clone(), "m": ts.m.clone(), "v": ts.v.clone()}
    x = obs["x"].clone()
    x[0, 0, 3, 5] = float("nan")
    out = ts.step(**dict(obs, x=x))
    st = ts.stats()
    assert math.isnan(float(out["loss"])) and st["n_skipped"] == 1 and st["skipped_last"] and st["opt_steps"] == 2
    for k, v in (("p", ts._on.flat_p), ("ema", ts._ema.flat_p), ("m", ts.m), ("v", ts.v)):
        assert torch.equal(_bits(v), _bits(before[k])), k
    assert math.isfinite(float(ts.step(**obs)["loss"])) and ts.stats()["opt_steps"] == 3


# ------------------------------------------------------------------------------------------------ 4. learning
def test_twenty_steps_learn_a_fixed_batch():
    ts, pred, obs = _fresh("l", lr=1e-3, p_dropout=0.0)
    sd = {k: v.detach().cpu().clone() for k, v in pred.state_dict().items()}
    l0 = float(ts.step(**obs)["loss"])
    for _ in range(19):
        ts.step(**obs)
    l20 = float(ts.loss_and_grads(**obs)[0])
    ref = T.f64_loop(sd, obs, 20, 1e-3)
    L = ref[-1]
    print(f"(32, 4): loss {l0:.4f} -> {l20:.4f} after 20 steps (f64 torch loop: {ref[0]:.4f} -> {L:.4f})")
    assert math.isfinite(l20) and L < l0
    assert l20 <= l0 - 0.5 * (l0 - L), (l0, l20, L)


# ------------------------------------------------------------------------------------------------ 5. determinism and capture
def _three_steps(tag, **kw):
    ts, pred, obs = _fresh(tag, lr=1e-3, ema_update_after=0, **kw)
    losses = [ts.step(**obs)["loss"] for _ in range(3)]
    torch.cuda.synchronize()
    return ts, dict(loss=torch.stack(losses), p=ts._on.flat_p, ep=ts._ema.flat_p, m=ts.m, v=ts.v, state=ts.state, g=ts.flat_g,
                    rng=ts._rng.float())


def test_fresh_instances_agree_bit_for_bit_and_the_captured_step_equals_the_eager_one():
    ta, a = _three_steps("b", use_graph=True)
    tb, b = _three_steps("b", use_graph=True)
    te, e = _three_steps("b", use_graph=False)
    assert ta.p_dropout == P and len(ta._graphs) == 1 and not te._graphs
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
        assert torch.equal(_bits(a[k]), _bits(e[k])), k
    assert not torch.equal(a["p"], a["ep"])  # (the weights moved and the EMA averaged)


# ------------------------------------------------------------------------------------------------ 6. eval sees training
def test_eval_sees_the_trained_weights_and_the_checkpoint_round_trips():
    from causal_gen_amd.predictor_resnet import ChestPredictor

    ts, pred, obs = _fresh("b", lr=1e-2, ema_update_after=0)
    full = {k: v.cuda() for k, v in obs.items()}
    before = pred.predict(**full)  # (builds the weight images: the cache the step must drop)
    before_ema = ts.ema_model.predict(**full)
    for _ in range(2):
        ts.step(**obs)
        pred.predict(**full)
    ts.step(**obs)
    assert not pred.training and not ts.ema_model.training
    sd = ts.state_dict()
    assert {"model_state_dict", "ema_model_state_dict", "optimizer_state_dict", "step"} <= set(sd)
    assert set(sd["model_state_dict"]) == set(pred.state_dict()) == set(sd["ema_model_state_dict"])
    assert len([k for k in sd["model_state_dict"] if k.split(".")[0].startswith("encoder_")]) == 248
    for model, key, old in ((pred, "model_state_dict", before), (ts.ema_model, "ema_model_state_dict", before_ema)):
        got = model.predict(**full)
        assert all(float((got[v] - old[v]).abs().max()) > 1e-5 for v in got), key
        fresh = ChestPredictor(SimpleNamespace(input_channels=1, input_res=33, std_fixed=0.0))
        fresh.load_reference_state_dict(sd[key])
        want = fresh.cuda().predict(**full)
        for v in got:
            assert torch.equal(_bits(got[v]), _bits(want[v])), (key, v)
    assert not torch.equal(pred.predict(**full)["race"], ts.ema_model.predict(**full)["race"])
    # the round trip: the next step is bit-identical on both sides
    other = _pred(33, seed=9)
    other.load_state_dict(sd["model_state_dict"], strict=True)
    torch.manual_seed(77)  # (another seed: the Philox state comes from the checkpoint)
    from causal_gen_amd.predictor_resnet_train import ChestPredictorTrainStep

    ts2 = ChestPredictorTrainStep(other, lr=1e-2, ema_update_after=0)
    ts2.load_state_dict(sd)
    la, lb = ts.step(**obs), ts2.step(**obs)
    torch.cuda.synchronize()
    assert torch.equal(_bits(la["loss"]), _bits(lb["loss"])) and torch.equal(_bits(la["grad_norm"]), _bits(lb["grad_norm"]))
    assert ts.it == ts2.it == 4
    for a, b in ((ts._on.flat_p, ts2._on.flat_p), (ts._ema.flat_p, ts2._ema.flat_p), (ts.m, ts2.m), (ts.v, ts2.v), (ts.state, ts2.state),
                 (ts._rng.float(), ts2._rng.float())):
        assert torch.equal(_bits(a), _bits(b))


def test_the_predictor_itself_stays_frozen_outside_the_step():
    ts, pred, obs = _fresh("a")
    with pytest.raises(NotImplementedError):
        pred._heads()
    assert pred.train().training is False
    with pytest.raises(ValueError, match="p_dropout"):
        _step(_pred(32), p_dropout=1.0)
    with pytest.raises(ValueError, match="input_res"):
        ts.step(**make_obs(2, 64, 0))
    with pytest.raises(KeyError, match="age"):
        ts.step(**{k: v for k, v in obs.items() if k != "age"})
    assert ts.it == 0 and not ts._graphs


# ------------------------------------------------------------------------------------------------ 7. step_from
COLS = {"sex": 0, "race": (1, 3), "finding": 4, "age": 5}


def _ds():
    from causal_gen_amd.data import DeviceDataset

    g = torch.Generator().manual_seed(0)
    x = torch.randint(0, 256, (16, 1, 32, 32), generator=g, dtype=torch.uint8)
    race = F.one_hot(torch.randint(0, 3, (16,), generator=g), 3).float()
    pa = torch.cat([torch.randint(0, 2, (16, 1), generator=g).float(), race, torch.randint(0, 2, (16, 1), generator=g).float(),
                    torch.rand(16, 1, generator=g) * 2 - 1], dim=1)
    return DeviceDataset(x, pa, 32, pad=(2, 2), hflip=0.5)


def _state(ts):
    out = dict(p=ts._on.flat_p, ep=ts._ema.flat_p, m=ts.m, v=ts.v, state=ts.state, g=ts.flat_g)
    for k, v in ts.model.state_dict().items():
        out["sd." + k] = v.float()
    return out


@pytest.mark.parametrize("graph", (True, False), ids=("captured", "eager"))
def test_step_from_equals_step_on_the_same_batch(graph):
    kw = dict(lr=1e-3, ema_update_after=0, use_graph=graph)
    ds = _ds()
    ts = _step(_pred(32), columns=COLS, **kw)
    twin = _step(_pred(32), **kw)
    B = 5
    d = torch.full((B, 3), -7, dtype=torch.int32, device="cuda")
    seen = []
    for i, idx in enumerate(([3, 11, 3, 0, 15], [1, 2, 2, 14, 9], [8, 8, 4, 5, 6])):  # (each with a repeated row)
        index = torch.tensor(idx, device="cuda")
        out = ts.step_from(ds, index, draws_out=d)
        torch.cuda.synchronize()
        assert len(ts._graphs) == (1 if graph else 0)  # another index replays the same graph
        seen.append(d.clone())
        my, mx = ds.draw_range()
        assert bool(((d[:, 0] >= 0) & (d[:, 0] <= my) & (d[:, 1] >= 0) & (d[:, 1] <= mx) & (d[:, 2] >= 0) & (d[:, 2] <= 1)).all())
        rows = ds.pa[index]
        obs = {var: rows[:, c:c + 1] if isinstance(c, int) else rows[:, c[0]:c[0] + c[1]] for var, c in COLS.items()}
        want = twin.step(x=ds.batch(index, draws=d)["x"], **obs)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out["loss"]), _bits(want["loss"])) and torch.equal(_bits(out["grad_norm"]), _bits(want["grad_norm"])), i
        got, ref = _state(ts), _state(twin)
        for k in got:
            assert torch.equal(_bits(got[k]), _bits(ref[k])), (i, k)
    assert ts.it == 3 and ts.stats()["opt_steps"] == 3 and int(ts._rng[1]) == 3
    assert not all(torch.equal(seen[0], s) for s in seen[1:])  # fresh draws on every replay
    with pytest.raises(ValueError, match="name the columns"):
        twin.step_from(ds, torch.tensor([0, 1], device="cuda"))
