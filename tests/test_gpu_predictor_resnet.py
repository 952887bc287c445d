"""ChestPredictor on the GPU against the f64 restatement (tests/resnet_ref.py).

A ReLU input within rounding of zero can take different branches in f32 and f64, and one such unit deep in the trunk moves the
whole input gradient by ~1e-2 (LABNOTES: with 4e5 .. 3e6 ReLU inputs of unit scale per case some input always lies within 1e-6
of zero).  So the gradient is compared with the oracle in PINNED mode -- every ReLU mask and the max pool's indices taken from
the activations the device computed -- and the pinning is itself checked: wherever the device's mask differs from the free
oracle's, the free oracle's pre-activation must lie within the activation tolerance of zero.

Tolerances.  Activations: per site, max error relative to the site's max <= max(1e-5, 4 x e_ref), e_ref = the error of torch's
own f32 run of the restatement at that site on that input (the arithmetic the reference uses; 4 x for another summation order
through 20 layers; 1e-5 = the project's tolerance for predictor outputs).  Loss and terms: 1e-5 relative (of max(1, |ref|), as
in test_gpu_predictor_tiled.py).  predict(): 1e-5 absolute.  Input gradient: 1e-4 of its max."""
import copy
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from resnet_ref import EPS32, VARS, chest_ref, make_obs, predict_ref, randomise

pytestmark = pytest.mark.gpu

CASES = {"a": (64, 2), "b": (33, 3), "c": (32, 1), "d": (192, 2), "e": (224, 2)}
RUNS = [(t, "") for t in sorted(CASES)] + [("a", "saturated"), ("a", "std_fixed")]


def _make(tag, variant="", seed=0):
    from causal_gen_amd.predictor_resnet import ChestPredictor

    R, B = CASES[tag]
    std_fixed = 0.3 if variant == "std_fixed" else 0.0
    pred = randomise(ChestPredictor(SimpleNamespace(input_channels=1, input_res=R, std_fixed=std_fixed)), 100 + seed)
    if variant == "saturated":  # classifier heads whose probabilities hit torch's clamp
        with torch.no_grad():
            for enc in (pred.encoder_s, pred.encoder_r, pred.encoder_f):
                enc.fc.weight.mul_(1e3)
                enc.fc.bias.mul_(1e3)
    return pred.cuda(), make_obs(B, R, 200 + seed), std_fixed


def _device_run(pred, obs):
    full = {k: v.cuda() for k, v in obs.items()}
    x = full["x"].clone().requires_grad_(True)
    loss = pred.model_anticausal(**dict(full, x=x))
    (gx,) = torch.autograd.grad(2.5 * loss, x)
    acts = pred.trunk_activations()
    terms = pred.nll_terms(**full)
    outs = {k: v.clone() for k, v in pred.raw_outputs(**full).items()}
    return {"loss": loss.detach().clone(), "gx": gx.clone(), "acts": acts, "terms": {k: v.clone() for k, v in terms.items()}, "outs": outs}


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(b.abs().max()), 1e-30)


@functools.lru_cache(maxsize=None)
def _case(tag, variant=""):
    """One device run and its references, shared by the tests of a case: the free f64 oracle, torch's f32 run of the same
    restatement (the per-site yardstick e_ref) and the pinned f64 oracle's input gradient."""
    pred, obs, std_fixed = _make(tag, variant)
    dev = _device_run(pred, obs)
    sd = {k: v.detach().cpu() for k, v in pred.state_dict().items()}
    with torch.no_grad():
        free = chest_ref(sd, obs, std_fixed)
        f32 = chest_ref(sd, obs, std_fixed, dtype=torch.float32)
    acts = [a.cpu() for a in dev["acts"]]
    e_ref = [_rel(a, b) for a, b in zip(f32["acts"], free["acts"])]
    tol = [max(1e-5, 4 * e) for e in e_ref]
    masks = [(a > 0).double() for a in acts[:17]]
    pool_idx = F.max_pool2d(acts[0], 3, 2, 1, return_indices=True)[1]
    x64 = obs["x"].double().requires_grad_(True)
    pinned = chest_ref(sd, dict(obs, x=x64), std_fixed, masks=masks, pool_idx=pool_idx)
    (rg,) = torch.autograd.grad(2.5 * pinned["loss"], x64)
    return SimpleNamespace(pred=pred, obs=obs, std_fixed=std_fixed, dev=dev, free=free, acts=acts, e_ref=e_ref, tol=tol, masks=masks,
                           pool_idx=pool_idx, pinned=pinned, rg=rg)


@pytest.mark.parametrize("tag,variant", RUNS)
def test_activations_match_the_free_oracle(tag, variant):
    c = _case(tag, variant)
    assert c.pred.path(c.obs["x"]) == "resnet" and len(c.acts) == 18
    bad = []
    for i, (got, want) in enumerate(zip(c.acts, c.free["acts"])):
        assert got.shape == want.shape and got.dtype == torch.float32, i
        err = _rel(got, want)
        print(f"case {tag}{variant and ' ' + variant} site {i:2d} {tuple(got.shape)}: device {err:.3e}, torch f32 {c.e_ref[i]:.3e}, tolerance {c.tol[i]:.3e}")
        if not err <= c.tol[i]:
            bad.append((i, err, c.tol[i]))
    assert not bad, bad


@pytest.mark.parametrize("tag,variant", RUNS)
def test_loss_terms_and_predict_match_the_free_oracle(tag, variant):
    c = _case(tag, variant)
    ref = float(c.free["loss"])
    got = float(c.dev["loss"])
    print(f"case {tag}{variant and ' ' + variant}: loss {got:.6f}, oracle {ref:.6f}, rel err {abs(got - ref) / max(1.0, abs(ref)):.3e}")
    assert abs(got - ref) <= 1e-5 * max(1.0, abs(ref))
    for var in VARS:
        want = c.free["terms"][var]
        assert c.dev["terms"][var].shape == want.shape
        assert float((c.dev["terms"][var].cpu().double() - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max())), var
        assert _rel(c.dev["outs"][var].cpu(), c.free["outs"][var]) <= 1e-5, var
    assert abs(sum(float(v.double().sum()) for v in c.dev["terms"].values()) - got) <= 1e-6 * max(1.0, abs(got))
    full = {k: v.cuda() for k, v in c.obs.items()}
    probs, want = c.pred.predict(**full), predict_ref(c.free["outs"])
    assert set(probs) == set(VARS)
    for var in VARS:
        assert probs[var].shape == want[var].shape, var
        assert float((probs[var].cpu().double() - want[var]).abs().max()) <= 1e-5 * (1.0 if var != "age" else max(1.0, float(want[var].abs().max()))), var
    if variant == "saturated":
        lo = float(-torch.log(torch.tensor(EPS32, dtype=torch.float64)))
        n_lo = sum(int(((c.dev["terms"][v].cpu().double() - lo).abs() < 1e-5).sum()) for v in ("sex", "race", "finding"))
        assert n_lo > 0, "no head reached the lower clamp"


@pytest.mark.parametrize("tag,variant", RUNS)
def test_input_gradient_matches_the_pinned_oracle(tag, variant):
    c = _case(tag, variant)
    # the pinning is legitimate: a unit whose mask differs from the free oracle's has a free pre-activation within tolerance of zero
    flips = 0
    for i, (m, pre, act) in enumerate(zip(c.masks, c.free["pres"], c.free["acts"])):
        diff = m != (pre > 0).double()
        n = int(diff.sum())
        flips += n
        if n:
            worst = float(pre[diff].abs().max())
            assert worst <= c.tol[i] * float(act.abs().max()), (i, n, worst)
    free_idx = F.max_pool2d(c.free["acts"][0], 3, 2, 1, return_indices=True)[1]
    pool_diff = c.pool_idx != free_idx
    if bool(pool_diff.any()):  # a pinned window may pick another pixel only if the two values tie within tolerance
        stem = c.free["acts"][0].flatten(2)
        gap = (stem.gather(2, free_idx.flatten(2)) - stem.gather(2, c.pool_idx.flatten(2))).abs()
        assert float(gap.max()) <= c.tol[0] * float(stem.abs().max())
    err = _rel(c.dev["gx"].cpu(), c.rg)
    print(f"case {tag}{variant and ' ' + variant}: input gradient error {err:.3e} of its max {float(c.rg.abs().max()):.3e}; "
          f"pinned ReLU disagreements {flips}, pool disagreements {int(pool_diff.sum())}")
    assert c.dev["gx"].shape == c.obs["x"].shape and float(c.rg.abs().max()) > 0
    assert err <= 1e-4


def test_reruns_are_bit_identical_and_images_do_not_see_their_batch():
    c = _case("b")
    again = _device_run(c.pred, c.obs)
    for k in ("loss", "gx"):
        assert torch.equal(again[k], c.dev[k]), k
    for var in VARS:
        assert torch.equal(again["terms"][var], c.dev["terms"][var]) and torch.equal(again["outs"][var], c.dev["outs"][var]), var
    one = _device_run(c.pred, {k: v[:1] for k, v in c.obs.items()})  # image 0 alone: GroupNorm is per image, nothing may leak
    tol = max(c.tol)  # the activation tolerance
    e_out = max(float((one["outs"][v] - c.dev["outs"][v][:1]).abs().max()) / max(1.0, float(c.dev["outs"][v][:1].abs().max())) for v in VARS)
    e_gx = float((one["gx"] - c.dev["gx"][:1]).abs().max()) / float(c.dev["gx"][:1].abs().max())
    e_act = max(float((got - want[:1]).abs().max()) / float(want[:1].abs().max()) for got, want in zip(one["acts"], c.dev["acts"]))
    print(f"image 0 alone against image 0 of a batch of 3: outputs {e_out:.3e}, input gradient {e_gx:.3e}, activations {e_act:.3e} (tolerance {tol:.1e})")
    assert e_out <= tol and e_gx <= tol and e_act <= tol


def test_captured_forward_and_backward_replay_on_new_contents():
    from causal_gen_amd import step_tail

    pred, obs, _ = _make("a", seed=1)
    other = make_obs(2, 64, seed=77)
    B = 2
    static = {k: v.cuda().contiguous() for k, v in obs.items()}
    x = static["x"]
    coef = torch.full((1,), 2.5, device="cuda")
    run = pred._run(x, static, need_obs=True)

    def step(terms, outs, loss, dx):
        pred._fwd(run, terms, outs, loss)
        pred._bwd(run, coef, dx)

    new = lambda: (torch.zeros(B, 4, device="cuda"), torch.zeros(4, B, 16, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros_like(x))
    warm = new()
    step(*warm)  # the eager run of the same launches
    cap = new()
    graph, _ = step_tail.capture(lambda: step(*cap))
    for k, v in other.items():  # new contents in the captured buffers: image, observations, upstream coefficient
        static[k].copy_(v.cuda())
    coef.fill_(-0.75)
    graph.replay()
    torch.cuda.synchronize()
    eager = new()
    step(*eager)
    torch.cuda.synchronize()
    assert not torch.equal(eager[2], warm[2]) and not torch.equal(eager[3], warm[3])
    for got, want in zip(cap, eager):
        assert torch.equal(got, want)
    # and through autograd: the same bits as the plan run by hand
    xg = static["x"].clone().requires_grad_(True)
    loss = pred.model_anticausal(**dict(static, x=xg))
    (gx,) = torch.autograd.grad(-0.75 * loss, xg)
    assert torch.equal(loss.detach().reshape(1), eager[2]) and torch.equal(gx, eager[3])


def test_weights_refresh_after_an_in_place_change():
    pred, obs, _ = _make("c", seed=2)
    full = {k: v.cuda() for k, v in obs.items()}
    before = {k: v.clone() for k, v in pred.raw_outputs(**full).items()}
    frozen = copy.deepcopy(pred)
    assert "_rt" not in frozen.__dict__ and "_ws" not in frozen.__dict__
    with torch.no_grad():
        pred.encoder_s.resnet[5][0].conv1.weight[3, 5].mul_(-2.0)
        pred.encoder_s.resnet[6][1].bn2.bias.add_(0.5)
    after = pred.raw_outputs(**full)
    assert all(not torch.equal(after[v], before[v]) for v in VARS)
    sd = {k: v.detach().cpu() for k, v in pred.state_dict().items()}
    with torch.no_grad():
        ref = chest_ref(sd, obs)
    for var in VARS:
        assert _rel(after[var].cpu(), ref["outs"][var]) <= 1e-4, var  # (the new weights, not the old images)
    old = frozen.raw_outputs(**full)
    assert all(torch.equal(old[v], before[v]) for v in VARS)


@pytest.fixture(scope="module")
def chest_dscm():
    import pgm_cases as PC
    from causal_gen_amd import vae
    from causal_gen_amd.hps import setup_hparams
    from causal_gen_amd.pgm_cf import DevicePGM
    from causal_gen_amd.predictor_resnet import ChestPredictor
    from oracle import fullsize_recipe as FR

    hp = setup_hparams("mimic192", input_res=32, enc_arch="32b1d2,16b1d2,8b1d8,1b1", dec_arch="1b1,8b1,16b1,32b1", widths=[16, 32, 48, 64],
                       z_max_res=16, pad=0)
    hp.dataset = "mimic"
    hp.lmbda_init, hp.elbo_constraint, hp.damping, hp.std_fixed = 1.0, 2.0, 10.0, 0.0
    torch.manual_seed(7)
    m = vae.HVAE(hp)
    m.apply(FR.init_bias)
    FR.perturb(m)
    m.compute_dtype = "f32"
    m = m.cuda()
    scm = PC.make_pgm("chest", seed=0).cuda()
    g = torch.Generator().manual_seed(3)
    pred = randomise(ChestPredictor(hp), 11).cuda()
    B = 3
    pa = scm.sample(B, torch.Generator().manual_seed(5))
    x = ((torch.randint(0, 256, (B, 1, 32, 32), generator=g).float() - 127.5) / 127.5).cuda()
    return hp, m, DevicePGM(scm, hp), pred, {k: v.cuda() for k, v in pa.items()}, x


def test_dscm_forward_takes_the_chest_predictor_and_the_metrics_update_in_place(chest_dscm):
    from causal_gen_amd import cf_eval, dscm
    from causal_gen_amd.predictor import AnticausalELBO

    hp, m, dev_pgm, pred, pa, x = chest_dscm
    for p in m.parameters():
        p.requires_grad_(True)
    model = dscm.DSCM(hp, dev_pgm, pred, m).cuda()
    obs = dict(pa, x=x)
    do = {"sex": 1.0 - pa["sex"]}
    out = model(obs, do, elbo_fn=AnticausalELBO())
    aux = out["aux_loss"]
    assert torch.isfinite(aux) and torch.isfinite(out["loss"]).all()
    cfs = {k: v.detach() for k, v in out["cfs"].items()}
    direct = pred.model_anticausal(**cfs) / x.shape[0]
    assert torch.equal(direct.reshape(()), aux.detach().reshape(()))
    out["loss"].sum().backward()
    torch.cuda.synchronize()
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0 for g in grads)
    assert all(p.grad is None for p in pred.parameters()), "the predictor is frozen"

    acc = cf_eval.MetricAccumulator(cf_eval.chest_metric_specs(), capacity=16)
    # (targets with every class present, so that each ROC-AUC is defined on three rows)
    targets = {"sex": torch.tensor([[0.0], [1.0], [0.0]]).cuda(), "finding": torch.tensor([[1.0], [0.0], [1.0]]).cuda(),
               "race": torch.eye(3).cuda(), "age": cfs["age"].reshape(-1, 1)}
    acc.update_from(pred, targets=targets, x=cfs["x"], finding=cfs["finding"])
    res = acc.compute()
    keys = {"sex_rocauc", "sex_acc", "finding_rocauc", "finding_acc", "age_mae", "race_acc", "race_rocauc"}
    assert keys <= set(res) and all(res["n"][v] == x.shape[0] for v in VARS)
    assert all(res[k] == res[k] and abs(res[k]) != float("inf") for k in keys), res
    # the in-place raw rows give what predict()'s probabilities give
    probs = pred.predict(x=cfs["x"], finding=cfs["finding"])
    acc2 = cf_eval.MetricAccumulator(cf_eval.chest_metric_specs(raw=False), capacity=16)
    acc2.update(probs, targets)
    res2 = acc2.compute()
    for k in ("sex_acc", "finding_acc", "race_acc"):
        assert res[k] == res2[k], k
    assert abs(res["age_mae"] - res2["age_mae"]) <= 1e-4 * max(1.0, abs(res2["age_mae"]))
