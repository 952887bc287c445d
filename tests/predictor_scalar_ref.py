"""torch restatement (any dtype; f64 is the oracle) of the scalar predictor head in TRAINING mode: layers.py's MLP with
``F.batch_norm(..., training=True)`` and the Normal likelihood flow_pgm.py's model_anticausal gives encoder_a, plus the cases the
tests of the kernel run and the whole-predictor loss (image heads + age) of the step tests.  Parameters are leaves in a dict keyed
by the module's names, buffers a dict of clones the forward updates as nn.BatchNorm1d does."""
import functools

import torch
import torch.nn.functional as F

import predictor_train_ref as R
from predictor_ref import normal_nll, randomise

MOMENTUM, BN_EPS = R.MOMENTUM, R.BN_EPS
PARAMS = ("mlp.0.weight", "mlp.1.weight", "mlp.1.bias", "mlp.3.weight", "mlp.4.weight", "mlp.4.bias", "mlp.6.weight", "mlp.6.bias")
STATS = ("mlp.1.running_mean", "mlp.1.running_var", "mlp.4.running_mean", "mlp.4.running_var")
COUNTS = ("mlp.1.num_batches_tracked", "mlp.4.num_batches_tracked")


def mlp_fwd(P, Bf, pre, inp, training=True):
    """Raw outputs [n, 2] of the MLP whose parameters / buffers are P[pre + name] / Bf[pre + name]"""
    h = F.linear(inp, P[pre + "mlp.0.weight"])
    h = F.leaky_relu(R._bn(h, P, Bf, pre + "mlp.1", training), 0.01)
    h = F.linear(h, P[pre + "mlp.3.weight"])
    h = F.leaky_relu(R._bn(h, P, Bf, pre + "mlp.4", training), 0.01)
    return F.linear(h, P[pre + "mlp.6.weight"], P[pre + "mlp.6.bias"])


def head_loss_and_grads(mlp, inp, obs, dtype, tanh_loc=False, std_fixed=0.0, coef=1.0):
    """coef * sum of the terms, {parameter: its gradient}, {statistic: value after the forward}, counters, on the CPU in `dtype`"""
    P, Bf = R.train_state(mlp, dtype)
    loss = normal_nll(mlp_fwd(P, Bf, "", inp.to(dtype)), obs.to(dtype), tanh_loc, std_fixed)
    gs = torch.autograd.grad(coef * loss, [P[n] for n in PARAMS])
    return dict(loss=loss.detach(), grads=dict(zip(PARAMS, gs)), bufs={n: Bf[n] for n in STATS}, counts={n: Bf[n] for n in COUNTS})


# tag: (nin, w, n, shift added to the inputs, std_fixed, tanh_loc, seed)
CASES = {
    "n4": (2, 32, 4, 0.0, 0.0, 0, 0),        # one partial wave
    "n5": (2, 32, 5, 0.0, 0.0, 0, 1),        # odd
    "n33": (2, 32, 33, 0.0, 0.0, 0, 2),      # more rows than row groups: a second tile with one row
    "n257": (2, 32, 257, 0.0, 0.0, 0, 3),    # several tiles
    "n1024": (2, 32, 1024, 0.0, 0.0, 0, 0),  # the largest batch a user trains at
    "shift8": (2, 32, 5, 8.0, 0.0, 0, 1),    # means far above the spread: fails a sum / sum-of-squares variance
    "std_fixed": (2, 32, 5, 0.0, 0.3, 0, 1),  # the logscale row's gradient is exactly zero
    "tanh": (2, 32, 5, 0.0, 0.0, 1, 1),
    # (one input: BatchNorm makes the output independent of |mlp.0.weight|, whose gradient is zero but for BatchNorm's eps -- every
    # draw is ill-conditioned in that tensor; torch's own f32 error is 2.3e-5 at this seed, 5e-5 to 6e-4 at seeds 0, 1, 2, 4..7)
    "nin1_w8": (1, 8, 5, 0.0, 0.0, 0, 3),
    "nin3_w64": (3, 64, 5, 0.0, 0.0, 0, 1),
}


def make_case(tag):
    """(MLP on the CPU with random weights and statistics, inputs [n, nin], target [n, 1]); inputs and target uniform on [-0.8, 0.8]"""
    from causal_gen_amd.predictor import MLP

    nin, w, n, shift, std_fixed, tanh_loc, seed = CASES[tag]
    g = torch.Generator().manual_seed(seed)
    mlp = MLP(nin, w, 2)
    randomise(mlp, g)
    inp = torch.rand(n, nin, generator=g) * 1.6 - 0.8 + shift
    obs = torch.rand(n, 1, generator=g) * 1.6 - 0.8
    return mlp, inp, obs


def _errors(r32, r64):
    e = {"loss": abs(float(r32["loss"]) - float(r64["loss"])) / max(1.0, abs(float(r64["loss"])))}
    for k in ("grads", "bufs"):
        for n in r64[k]:
            e[n] = R.rel_err(r32[k][n], r64[k][n])
    return e


@functools.lru_cache(maxsize=None)
def reference(tag):
    """f64 oracle of a case and e32 = the error of torch's own f32 CPU run against it, per tensor"""
    mlp, inp, obs = make_case(tag)
    _, _, _, _, std_fixed, tanh_loc, _ = CASES[tag]
    r64 = head_loss_and_grads(mlp, inp, obs, torch.float64, bool(tanh_loc), std_fixed)
    r32 = head_loss_and_grads(mlp, inp, obs, torch.float32, bool(tanh_loc), std_fixed)
    return mlp, inp, obs, r64, _errors(r32, r64)


# ---- the whole FlowPredictor: image heads (predictor_train_ref.image_nll) + the age term
def full_nll(pred, P, Bf, obs, training=True):
    B = obs["x"].shape[0]
    total = R.image_nll(pred, P, Bf, obs, training)
    for sh in pred._scalar_heads():
        pre = next(n for n, m in pred.named_modules() if m is sh.mlp) + "."
        inp = torch.cat([obs[v].reshape(B, -1) for v in sh.inputs], dim=-1)
        total = total + normal_nll(mlp_fwd(P, Bf, pre, inp, training), obs[sh.var], sh.tanh_loc, float(pred.std_fixed))
    return total


def full_loss_and_grads(pred, obs, dtype):
    """mean loss, {every named parameter: gradient}, {every float buffer: value after the forward}, counters"""
    P, Bf = R.train_state(pred, dtype)
    o = {k: v.detach().cpu().to(dtype) for k, v in obs.items()}
    loss = full_nll(pred, P, Bf, o) / o["x"].shape[0]
    names = [n for n, _ in pred.named_parameters()]
    gs = torch.autograd.grad(loss, [P[n] for n in names])
    return dict(loss=loss.detach(), grads=dict(zip(names, gs)), bufs={n: b for n, b in Bf.items() if b.is_floating_point()},
                counts={n: b for n, b in Bf.items() if not b.is_floating_point()})


@functools.lru_cache(maxsize=None)
def full_reference(tag):
    pred, obs = R.make_case(tag)
    r64, r32 = full_loss_and_grads(pred, obs, torch.float64), full_loss_and_grads(pred, obs, torch.float32)
    return pred, obs, r64, _errors(r32, r64)
