"""Time the anticausal predictors: forward (loss) and forward + d/dx, HIP vs torch eager on the same GPU (the same eval-mode CNNs,
torch.distributions, autograd.grad w.r.t. x).  Cases: morphomnist and cmnist at B = 256 (fused, and the workspace path forced
with CGEN_PREDICTOR_LAYERED=1; morphomnist also through the tiled path, for information), ukbb192 at B = 32 (workspace path and
tiled path, the default there).  Prints one JSON line per case; each row times its own eager columns."""
import json
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from causal_gen_amd import predictor as P  # noqa: E402
from predictor_ref import randomise  # noqa: E402


def obs_for(ds, B, C, R, g):
    x = ((torch.rand(B, C, R, R, generator=g) * 2 - 1) * 1.3).clamp(-1, 1)
    oh = lambda: torch.nn.functional.one_hot(torch.randint(0, 10, (B,), generator=g), 10).float()
    u = lambda: torch.rand(B, 1, generator=g) * 1.6 - 0.8
    if ds == "morphomnist":
        o = {"thickness": u(), "intensity": u(), "digit": oh()}
    elif ds == "cmnist":
        o = {"digit": oh(), "colour": oh()}
    else:
        o = {"sex": (u() > 0).float(), "mri_seq": (u() > 0).float(), "age": u(), "brain_volume": u(), "ventricle_volume": u()}
    return {k: v.cuda() for k, v in dict(o, x=x).items()}


def timeit(fn, warm=3, reps=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def eager_model(pred):
    """The eval-mode modules' own torch layers in f32 (eager): the reference CNN's forward, BN unfolded."""
    def fwd(cnn, x, y=None):
        h = cnn.cnn(x).mean(dim=(-2, -1))
        if y is not None:
            h = torch.cat([h, y], -1)
        return cnn.fc(h)
    return fwd


def eager_nll(pred, obs):
    fwd = eager_model(pred)
    x, B = obs["x"], obs["x"].shape[0]
    F = torch.nn.functional
    D = torch.distributions
    f = lambda ls: F.softplus(ls)
    if isinstance(pred, P.MorphoMNISTPredictor):
        tl, ts = fwd(pred.encoder_t, x, obs["intensity"]).chunk(2, -1)
        il, is_ = fwd(pred.encoder_i, x).chunk(2, -1)
        return -(D.Normal(torch.tanh(tl), f(ts)).log_prob(obs["thickness"]).sum() + D.Normal(torch.tanh(il), f(is_)).log_prob(obs["intensity"]).sum()
                 + D.OneHotCategorical(probs=F.softmax(fwd(pred.encoder_y, x), -1)).log_prob(obs["digit"]).sum())
    if isinstance(pred, P.ColourMNISTPredictor):
        return -(D.OneHotCategorical(probs=F.softmax(fwd(pred.encoder_y, x), -1)).log_prob(obs["digit"]).sum()
                 + D.OneHotCategorical(probs=F.softmax(fwd(pred.encoder_c, x), -1)).log_prob(obs["colour"]).sum())
    vl, vs = fwd(pred.encoder_v, x).chunk(2, -1)
    bl, bs = fwd(pred.encoder_b, x, obs["ventricle_volume"]).chunk(2, -1)
    al, as_ = pred.encoder_a(torch.cat([obs["brain_volume"], obs["ventricle_volume"]], -1)).chunk(2, -1)
    return -(D.Normal(vl, f(vs)).log_prob(obs["ventricle_volume"]).sum() + D.Normal(bl, f(bs)).log_prob(obs["brain_volume"]).sum()
             + D.Normal(al, f(as_)).log_prob(obs["age"]).sum()
             + D.Bernoulli(probs=torch.sigmoid(fwd(pred.encoder_s, x, obs["brain_volume"]))).log_prob(obs["sex"]).sum()
             + D.Bernoulli(probs=torch.sigmoid(fwd(pred.encoder_m, x))).log_prob(obs["mri_seq"]).sum())


def main():
    cases = [("morphomnist", 1, 32, 256, "fused"), ("morphomnist", 1, 32, 256, "workspace"), ("morphomnist", 1, 32, 256, "tiled"),
             ("cmnist", 3, 32, 256, "fused"), ("cmnist", 3, 32, 256, "workspace"), ("ukbb192", 1, 192, 32, "workspace"),
             ("ukbb192", 1, 192, 32, "tiled")]
    for ds, C, R, B, path in cases:
        os.environ["CGEN_PREDICTOR_LAYERED"] = "1" if path == "workspace" else "0"
        os.environ["CGEN_PREDICTOR_TILED"] = "1" if path == "tiled" else "0"
        g = torch.Generator().manual_seed(0)
        pred = P.make_predictor(SimpleNamespace(dataset=ds, input_channels=C, input_res=R, std_fixed=0.0))
        randomise(pred, g)
        pred = pred.cuda()
        obs = obs_for(ds, B, C, R, g)
        assert pred.path(obs["x"]) == path, (pred.path(obs["x"]), path)

        def hip_fwd():
            with torch.no_grad():
                pred.model_anticausal(**obs)

        def hip_fb():
            x = obs["x"].detach().requires_grad_(True)
            torch.autograd.grad(pred.model_anticausal(**dict(obs, x=x)), x)

        def eager_fwd():
            with torch.no_grad():
                eager_nll(pred, obs)

        def eager_fb():
            x = obs["x"].detach().requires_grad_(True)
            torch.autograd.grad(eager_nll(pred, dict(obs, x=x)), x)

        row = {"case": ds, "B": B, "path": path, "hip_fwd_ms": round(timeit(hip_fwd), 4),
               "hip_fwd_bwd_ms": round(timeit(hip_fb), 4), "eager_fwd_ms": round(timeit(eager_fwd), 4),
               "eager_fwd_bwd_ms": round(timeit(eager_fb), 4)}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
