"""The tiled placement of the anticausal predictors on the MI355X (one launch per layer over tile x image x head): loss and
d aux / dx against the f64 oracle, head outputs against the reference CNN's fixtures, saturated heads, determinism and batch
independence, routing, the autograd tape and hipGraph capture."""
import copy
import ctypes
from types import SimpleNamespace

import pytest
import torch

from conftest import load_golden
from predictor_ref import EPS32, cnn_ref, predictor_nll, randomise
from test_gpu_predictor import _check_saturated_heads, _obs

pytestmark = pytest.mark.gpu

CASES = {
    # tag: (dataset, C, R, B): the smallest shapes that reach every branch of the tiled kernels
    "a": ("ukbb192", 1, 192, 2),  # stride-2 stem, pool, 96 / 48 / 24 / 12 / 6
    "b": ("ukbb192", 1, 66, 3),   # odd h1 = 33: the pool drops the last row and column; 16 / 8 / 4 / 2
    "c": ("cmnist", 3, 40, 3),    # pool behind a stride-1 stem, 3 input channels; 20 / 10 / 5 / 3
    "d": ("morphomnist", 1, 32, 5),  # no pool; the fused path takes the same input
    "e": ("ukbb192", 1, 9, 2),    # smaller than any tile: 9 / 5 / 3 / 2
}


@pytest.fixture(autouse=True)
def tiled(monkeypatch):
    monkeypatch.setenv("CGEN_PREDICTOR_TILED", "1")
    monkeypatch.setenv("CGEN_PREDICTOR_LAYERED", "0")


def _make(tag, seed=0, std_fixed=0.0, scale=1.0, shape=None):
    from causal_gen_amd import predictor as P

    ds, C, R, B = CASES[tag]
    if shape:
        C, R, B = shape
    g = torch.Generator().manual_seed(seed)
    pred = P.make_predictor(SimpleNamespace(dataset=ds, input_channels=C, input_res=R, std_fixed=std_fixed))
    randomise(pred, g)
    with torch.no_grad():  # saturating classifier heads: their probabilities hit torch's clamp
        for name in ("encoder_y", "encoder_c", "encoder_s", "encoder_m"):
            if hasattr(pred, name):
                getattr(pred, name).fc[3].weight.mul_(scale)
                getattr(pred, name).fc[3].bias.mul_(scale)
    return pred.cuda(), _obs("ukbb" if "ukbb" in ds else ds, B, C, R, g)


def _loss_grad(pred, obs, coef=2.5):
    x = obs["x"].cuda().requires_grad_(True)
    loss = pred.model_anticausal(**dict(obs, x=x))
    (gx,) = torch.autograd.grad(coef * loss, x)
    return loss.detach(), gx


_REF = {}


def _oracle(key, pred, obs, std_fixed):
    if key not in _REF:
        x64 = obs["x"].double().cuda().requires_grad_(True)
        ref = predictor_nll(pred, dict(obs, x=x64), std_fixed)
        (rg,) = torch.autograd.grad(2.5 * ref, x64)
        _REF[key] = (ref.item(), rg)
    return _REF[key]


def _errors(pred, obs, ref, rg):
    loss, gx = _loss_grad(pred, obs)
    return abs(loss.item() - ref) / max(1.0, abs(ref)), (gx.double() - rg).abs().max().item() / max(rg.abs().max().item(), 1e-30)


@pytest.mark.parametrize("tag,std_fixed", [(t, 0.0) for t in sorted(CASES)] + [("d", 0.3)])
def test_tiled_loss_and_input_gradient_match_f64_oracle(tag, std_fixed, monkeypatch):
    pred, obs = _make(tag, std_fixed=std_fixed)
    assert pred.path(obs["x"]) == "tiled"
    ref, rg = _oracle((tag, std_fixed), pred, obs, std_fixed)
    el, eg = _errors(pred, obs, ref, rg)
    print(f"case {tag} std_fixed {std_fixed}: tiled loss rel err {el:.3e}, grad rel err {eg:.3e}")
    if tag in ("a", "d"):  # for the record: the workspace path on the same inputs
        monkeypatch.setenv("CGEN_PREDICTOR_LAYERED", "1")
        assert pred.path(obs["x"]) == "workspace"
        wl, wg = _errors(pred, obs, ref, rg)
        print(f"case {tag} std_fixed {std_fixed}: workspace loss rel err {wl:.3e}, grad rel err {wg:.3e}")
    assert el <= 1e-5, (tag, el)
    assert eg <= 1e-4, (tag, eg)


@pytest.mark.parametrize("tag", ["morphomnist"] + [f"ukbb192_encoder_{h}" for h in "vbsm"])
def test_tiled_head_outputs_match_reference_cnn(tag):
    from causal_gen_amd.predictor import CNN

    gd = load_golden(f"predictor_{tag}.pt")
    for name, h in gd["heads"].items():
        cnn = CNN(gd["in_shape"], width=h["width"], num_outputs=h["nout"], context_dim=h["ctx"])
        cnn.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in h["state_dict"].items()}, strict=True)
        x = gd["x"].float().cuda()
        assert cnn.path(x) == "tiled"
        out = cnn(x, h["y"].cuda() if h["y"] is not None else None).cpu().double()
        err = (out - h["out64"]).abs().max() / h["out64"].abs().max()
        assert err < 1e-5, (name, err.item())


@pytest.mark.parametrize("width", [32, 24])
def test_tiled_bare_cnn_of_other_widths_matches_f64(width):
    from causal_gen_amd.predictor import CNN

    g = torch.Generator().manual_seed(11)
    cnn = CNN((1, 72, 72), width=width, num_outputs=3)
    randomise(cnn, g)
    x = _obs("cmnist", 2, 1, 72, g)["x"]
    assert cnn.path(x.cuda()) == "tiled"
    out = cnn(x.cuda()).cpu().double()
    want = cnn_ref(cnn, x.double())
    err = (out - want).abs().max() / want.abs().max()
    assert err < 1e-5, (width, err.item())


def test_tiled_saturated_bernoulli_heads_cost_minus_log_eps():
    pred, obs = _make("a", scale=1e3)
    terms = pred.nll_terms(**{k: v.cuda() for k, v in obs.items()})
    lo = float(-torch.log(torch.tensor(EPS32, dtype=torch.float64)))
    t = torch.cat([terms["sex"], terms["mri_seq"]]).double().cpu()
    assert int(((t - lo).abs() < 1e-5).sum()) >= 1, t


def test_tiled_saturated_cmnist_heads_give_no_gradient():
    pred, obs = _make("c", scale=1e3, shape=(3, 32, 4))  # the existing cmnist_saturated case: same seed, same draws
    assert pred.path(obs["x"]) == "tiled"
    ref, rg = _oracle("cmnist_saturated", pred, obs, 0.0)
    loss, gx = _loss_grad(pred, obs)
    assert abs(loss.item() - ref) <= 1e-5 * max(1.0, abs(ref))
    assert (gx.double() - rg).abs().max().item() <= 1e-4 * max(rg.abs().max().item(), 1e-30)
    _check_saturated_heads(pred, obs, gx)  # >= 1 sample with every head clamped, and dx == 0 exactly there


@pytest.mark.parametrize("tag", ["a", "c"])
def test_tiled_is_deterministic_and_independent_of_the_batch(tag):
    pred, obs = _make(tag, seed=3)
    runs = [_loss_grad(pred, obs, coef=1.0) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    cu = {k: v.cuda() for k, v in obs.items()}
    full = {k: v.clone() for k, v in pred.nll_terms(**cu).items()}
    one = {k: v[1:2].contiguous() for k, v in obs.items()}
    alone = pred.nll_terms(**{k: v.cuda() for k, v in one.items()})
    for k in full:
        assert torch.equal(full[k][1:2], alone[k]), k
    _, g1 = _loss_grad(pred, one, coef=1.0)
    assert torch.equal(runs[0][1][1:2], g1)


def test_routing(monkeypatch):
    from causal_gen_amd import predictor as P

    mk = lambda ds, R: P.make_predictor(SimpleNamespace(dataset=ds, input_channels=1, input_res=R, std_fixed=0.0)).cuda()
    preds = {32: mk("morphomnist", 32), 64: mk("ukbb64", 64), 192: mk("ukbb192", 192)}  # (the 32x32 preset; width-16 heads do not fit LDS)
    xs = {R: torch.zeros(2, 1, R, R, device="cuda") for R in preds}
    monkeypatch.delenv("CGEN_PREDICTOR_TILED")
    monkeypatch.delenv("CGEN_PREDICTOR_LAYERED")
    assert [preds[R].path(xs[R]) for R in (32, 192, 64)] == ["fused", "tiled", "tiled"]
    monkeypatch.setenv("CGEN_PREDICTOR_LAYERED", "1")
    assert [preds[R].path(xs[R]) for R in (32, 192, 64)] == ["workspace"] * 3
    monkeypatch.delenv("CGEN_PREDICTOR_LAYERED")
    monkeypatch.setenv("CGEN_PREDICTOR_TILED", "0")
    assert preds[192].path(xs[192]) == "workspace"
    assert preds[32].path(xs[32]) == "fused"
    monkeypatch.setenv("CGEN_PREDICTOR_TILED", "1")
    assert preds[32].path(xs[32]) == "tiled"
    assert preds[192].encoder_v.path(xs[192]) == "tiled"


def test_predict_on_the_default_route_matches_reference_transforms(monkeypatch):
    monkeypatch.delenv("CGEN_PREDICTOR_TILED")
    monkeypatch.delenv("CGEN_PREDICTOR_LAYERED")
    pred, obs = _make("a", seed=5)
    ema = copy.deepcopy(pred)
    assert ema.path(obs["x"]) == "tiled" and "_ws_tiled" not in ema.__dict__
    out = ema.predict(**{k: v.cuda() for k, v in obs.items()})
    x = obs["x"].double().cuda()
    o = {k: v.double().cuda() for k, v in obs.items()}
    want = {"sex": torch.sigmoid(cnn_ref(pred.encoder_s, x, o["brain_volume"])), "mri_seq": torch.sigmoid(cnn_ref(pred.encoder_m, x)),
            "brain_volume": cnn_ref(pred.encoder_b, x, o["ventricle_volume"])[:, :1], "ventricle_volume": cnn_ref(pred.encoder_v, x)[:, :1]}
    for k, v in want.items():
        assert (out[k].double() - v).abs().max() <= 1e-5 * max(1.0, v.abs().max().item()), k
    assert "age" in out


def test_backward_uses_the_path_of_its_forward(monkeypatch):
    pred, obs = _make("b", seed=2)
    x = obs["x"].cuda().requires_grad_(True)
    loss = pred.model_anticausal(**dict(obs, x=x))
    monkeypatch.setenv("CGEN_PREDICTOR_LAYERED", "1")  # the environment changes between forward and backward
    (gx,) = torch.autograd.grad(loss, x)
    monkeypatch.setenv("CGEN_PREDICTOR_LAYERED", "0")
    _, want = _loss_grad(pred, obs, coef=1.0)
    assert torch.equal(gx, want)


def test_anticausal_elbo_is_the_model_loss_on_one_tape():
    from causal_gen_amd.predictor import AnticausalELBO

    pred, obs = _make("a", seed=7)
    res = []
    for fn in (lambda **c: AnticausalELBO().differentiable_loss(pred.model_anticausal, pred.guide_pass, **c), pred.model_anticausal):
        x = obs["x"].cuda().requires_grad_(True)
        loss = fn(**dict({k: v.cuda() for k, v in obs.items()}, x=x))
        (gx,) = torch.autograd.grad(loss, x)
        res.append((loss.detach(), gx))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_tiled_entry_points_capture_into_one_graph():
    from causal_gen_amd import _lib
    from causal_gen_amd import predictor as P

    lib = _lib.require_gpu()
    pred, obs = _make("b", seed=4)
    heads = pred._heads()
    full = {k: v.cuda() for k, v in obs.items()}
    x = P._prep_x(full["x"])
    B, nh = x.shape[0], len(heads)
    recs, keep = P._records(heads, dict(full, x=x), 0.0, need_obs=True)
    need = _lib.i64(0)
    lib.predictor_tiled_workspace(recs, nh, B, ctypes.byref(need))
    ws = torch.empty(need.value, device="cuda")
    coef = torch.ones(1, device="cuda")

    def run(terms, loss, dx):
        st = torch.cuda.current_stream().cuda_stream
        lib.predictor_tiled_fwd(recs, nh, B, x.data_ptr(), ws.data_ptr(), ws.numel(), terms.data_ptr(), None, loss.data_ptr(), st)
        lib.predictor_tiled_bwd(recs, nh, B, x.data_ptr(), ws.data_ptr(), ws.numel(), coef.data_ptr(), dx.data_ptr(), st)

    eager = (torch.empty(B, nh, device="cuda"), torch.empty(1, device="cuda"), torch.empty_like(x))
    run(*eager)  # the eager warm-up run, and the values to compare with
    torch.cuda.synchronize()
    cap = (torch.zeros(B, nh, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros_like(x))
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        run(*cap)
    for _ in range(2):
        for t in cap:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(cap, eager):
            assert torch.equal(got, want)
