"""Anticausal predictors on the MI355X: head outputs against the reference CNN (golden files), the loss and d aux / dx against
the f64 oracle (tests/predictor_ref.py), fused vs workspace path, determinism, predict()."""
import copy
import os
from types import SimpleNamespace

import pytest
import torch

from conftest import load_golden
from predictor_ref import EPS32, predictor_nll, randomise

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["fused", "layered"])
def path(request, monkeypatch):
    monkeypatch.setenv("CGEN_PREDICTOR_LAYERED", "1" if request.param == "layered" else "0")
    return request.param


@pytest.mark.parametrize("tag", ["morphomnist", "cmnist"] + [f"ukbb192_encoder_{h}" for h in "vbsm"])
def test_head_outputs_match_reference_cnn(tag, path):
    from causal_gen_amd.predictor import CNN

    gd = load_golden(f"predictor_{tag}.pt")
    for name, h in gd["heads"].items():
        cnn = CNN(gd["in_shape"], width=h["width"], num_outputs=h["nout"], context_dim=h["ctx"])
        cnn.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in h["state_dict"].items()}, strict=True)
        out = cnn(gd["x"].float().cuda(), h["y"].cuda() if h["y"] is not None else None).cpu().double()
        err = (out - h["out64"]).abs().max() / h["out64"].abs().max()
        assert err < 1e-5, (name, path, err.item())


def _obs(kind, B, C, R, g, saturate=False):
    x = ((torch.rand(B, C, R, R, generator=g) * 2 - 1) * 1.3).clamp(-1, 1)
    x[0, :, : R // 2] = -1.0  # constant background: exact ties in the max-pool windows
    x[:, :, :, : R // 8] = 1.0
    oh = lambda n: torch.nn.functional.one_hot(torch.randint(0, n, (B,), generator=g), n).float()
    if kind == "morphomnist":
        return {"x": x, "thickness": torch.rand(B, 1, generator=g) * 1.6 - 0.8, "intensity": torch.rand(B, 1, generator=g) * 1.6 - 0.8,
                "digit": oh(10)}
    if kind == "cmnist":
        return {"x": x, "digit": oh(10), "colour": oh(10)}
    return {"x": x, "sex": torch.randint(0, 2, (B, 1), generator=g).float(), "mri_seq": torch.randint(0, 2, (B, 1), generator=g).float(),
            "age": torch.rand(B, 1, generator=g) * 1.6 - 0.8, "brain_volume": torch.rand(B, 1, generator=g) * 1.6 - 0.8,
            "ventricle_volume": torch.rand(B, 1, generator=g) * 1.6 - 0.8}


CASES = {
    # tag: (dataset, C, R, B, logit scale of the categorical / Bernoulli heads, std_fixed)
    "morphomnist": ("morphomnist", 1, 32, 6, 1.0, 0.0),
    "morphomnist_std_fixed": ("morphomnist", 1, 32, 4, 1.0, 0.3),
    "morphomnist_saturated": ("morphomnist", 1, 32, 4, 1e3, 0.0),
    "cmnist": ("cmnist", 3, 32, 5, 1.0, 0.0),
    "cmnist_saturated": ("cmnist", 3, 32, 4, 1e3, 0.0),
    "ukbb64": ("ukbb64", 1, 64, 3, 1.0, 0.0),
    "ukbb192": ("ukbb192", 1, 192, 2, 1.0, 0.0),
    "ukbb192_saturated": ("ukbb192", 1, 192, 2, 1e3, 0.0),
}


def _make(tag, seed=0):
    from causal_gen_amd import predictor as P

    ds, C, R, B, scale, std_fixed = CASES[tag]
    g = torch.Generator().manual_seed(seed)
    pred = P.make_predictor(SimpleNamespace(dataset=ds, input_channels=C, input_res=R, std_fixed=std_fixed))
    randomise(pred, g)
    with torch.no_grad():  # saturating classifier heads: their probabilities hit torch's clamp
        for name in ("encoder_y", "encoder_c", "encoder_s", "encoder_m"):
            if hasattr(pred, name):
                getattr(pred, name).fc[3].weight.mul_(scale)
                getattr(pred, name).fc[3].bias.mul_(scale)
    return pred.cuda(), _obs("ukbb" if "ukbb" in ds else ds, B, C, R, g), std_fixed


@pytest.mark.parametrize("tag,layered", [(t, m) for t in sorted(CASES) for m in ("0", "1") if m == "1" or "ukbb" not in t])
def test_loss_and_input_gradient_match_f64_oracle(tag, layered, monkeypatch):
    # (the fused path takes the 32x32 presets; ukbb images run the workspace path)
    monkeypatch.setenv("CGEN_PREDICTOR_LAYERED", layered)
    pred, obs, std_fixed = _make(tag)
    x = obs["x"].cuda().requires_grad_(True)
    loss = pred.model_anticausal(**dict(obs, x=x))
    (gx,) = torch.autograd.grad(2.5 * loss, x)
    x64 = obs["x"].double().cuda().requires_grad_(True)
    ref = predictor_nll(pred, dict(obs, x=x64), std_fixed)
    (rg,) = torch.autograd.grad(2.5 * ref, x64)
    assert abs(loss.item() - ref.item()) <= 1e-5 * max(1.0, abs(ref.item())), (tag, loss.item(), ref.item())
    scale = rg.abs().max().item()
    assert (gx.double() - rg).abs().max().item() <= 1e-4 * max(scale, 1e-30), (tag, scale)
    if tag.endswith("saturated"):
        _check_saturated_heads(pred, obs, gx)


def _check_saturated_heads(pred, obs, gx):
    """The kernel's own per-sample terms of the classifier heads: a clamped probability costs exactly -log(eps) (or -log(1-eps))
    and contributes no gradient; a sample whose heads are all clamped gets dx == 0 exactly."""
    terms = pred.nll_terms(**{k: v.cuda() for k, v in obs.items()})
    lo = float(-torch.log(torch.tensor(EPS32, dtype=torch.float64)))  # 15.9424
    hi = float(-torch.log1p(torch.tensor(-EPS32, dtype=torch.float64)))  # 1.19e-7
    sat = {}
    for var in ("digit", "colour", "sex", "mri_seq"):
        if var in terms:
            t = terms[var].double().cpu()
            s_lo, s_hi = (t - lo).abs() < 1e-5, (t - hi).abs() < 1e-12
            sat[var] = s_lo | s_hi
    n_lo = sum(int(((terms[v].double().cpu() - lo).abs() < 1e-5).sum()) for v in sat)
    assert n_lo > 0, "no head reached the lower clamp"
    if not any(v in terms for v in ("thickness", "intensity", "brain_volume", "ventricle_volume")):
        all_sat = torch.stack(list(sat.values())).all(0)
        assert bool(all_sat.any()), "no sample with every head clamped"
        assert bool((gx[all_sat.cuda()] == 0).all()), "clamped heads must contribute no gradient"


@pytest.mark.parametrize("tag", ["morphomnist", "cmnist"])
def test_fused_and_workspace_paths_agree_and_are_deterministic(tag, monkeypatch):
    """The LDS and the global-workspace placements of the same kernel (and the workspace sizing) agree; reruns are bit-identical."""
    pred, obs, _ = _make(tag, seed=3)
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("CGEN_PREDICTOR_LAYERED", mode)
        runs = []
        for _ in range(2):
            x = obs["x"].cuda().requires_grad_(True)
            loss = pred.model_anticausal(**dict(obs, x=x))
            (gx,) = torch.autograd.grad(loss, x)
            runs.append((loss.detach().clone(), gx.clone()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), mode
        res[mode] = runs[0]
    assert torch.allclose(res["0"][0], res["1"][0], rtol=1e-6, atol=0)
    assert (res["0"][1] - res["1"][1]).abs().max() <= 1e-5 * res["1"][1].abs().max()


@pytest.mark.parametrize("tag", ["morphomnist", "cmnist", "ukbb192"])
def test_predict_matches_reference_transforms(tag):
    from predictor_ref import cnn_ref

    pred, obs, _ = _make(tag, seed=5)
    ema = copy.deepcopy(pred)  # train_cf.py:183 predicts with the EMA copy: runtime state is not copied, weights are
    out = ema.predict(**{k: v.cuda() for k, v in obs.items()})
    x = obs["x"].double().cuda()
    o = {k: v.double().cuda() for k, v in obs.items()}
    sm = lambda t: torch.softmax(t, -1)
    if tag == "morphomnist":
        want = {"thickness": torch.tanh(cnn_ref(pred.encoder_t, x, o["intensity"])[:, :1]),
                "intensity": torch.tanh(cnn_ref(pred.encoder_i, x)[:, :1]), "digit": sm(cnn_ref(pred.encoder_y, x))}
    elif tag == "cmnist":
        want = {"digit": sm(cnn_ref(pred.encoder_y, x)), "colour": sm(cnn_ref(pred.encoder_c, x))}
    else:
        want = {"sex": torch.sigmoid(cnn_ref(pred.encoder_s, x, o["brain_volume"])), "mri_seq": torch.sigmoid(cnn_ref(pred.encoder_m, x)),
                "brain_volume": cnn_ref(pred.encoder_b, x, o["ventricle_volume"])[:, :1],
                "ventricle_volume": cnn_ref(pred.encoder_v, x)[:, :1]}
    for k, v in want.items():
        assert (out[k].double() - v).abs().max() <= 1e-5 * max(1.0, v.abs().max().item()), k
    assert "age" in out if tag == "ukbb192" else True


def test_anticausal_elbo_is_the_model_loss():
    from causal_gen_amd.predictor import AnticausalELBO

    pred, obs, _ = _make("morphomnist", seed=7)
    cfs = {k: v.cuda() for k, v in obs.items()}
    a = AnticausalELBO().differentiable_loss(pred.model_anticausal, pred.guide_pass, **cfs)
    b = pred.model_anticausal(**cfs)
    assert torch.equal(a, b)
