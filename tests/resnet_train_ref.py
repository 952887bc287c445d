"""f64 references for ChestPredictorTrainStep on top of tests/resnet_ref.py: the loss and all 68 parameter gradients of loss / B
(plus d loss / dx) through autograd on ``chest_ref``, free or pinned, and the f64 AdamW / clip / EMA tail of one step.

Dropout needs no oracle code of its own: in pinned mode ``masks[a1 site] = keep_and_relu_mask / (1 - p)`` -- ``_MaskRelu``
multiplies forward and backward by whatever it is given.

``chest_ref`` detaches the tensors of the state dict it is handed (they are constants for the eval tests).  The parameters are
therefore passed as a tensor subclass whose ``detach()`` is the identity, so that autograd reaches the leaves behind them."""
import math

import torch

from resnet_ref import ENC, VARS, chest_ref

from oracle import train_ref

U = 2.0 ** -24
A1_SITES = tuple(1 + 2 * k for k in range(8))  # relu(bn1) of block k in the order of acts / masks


class _Attached(torch.Tensor):
    def detach(self):
        return self


def param_names(sd):
    """The 68 distinct parameter names in ``ChestPredictor.named_parameters()`` order: the one trunk under encoder_s, then the
    four fc pairs."""
    return [k for k in sd if k.startswith("encoder_s.resnet.")] + [f"{ENC[v]}.fc.{n}" for v in VARS for n in ("weight", "bias")]


def loss_and_grads_ref(sd, obs, std_fixed=0.0, masks=None, pool_idx=None, dtype=torch.float64):
    """dict(loss = sum of terms / B, grads = {name: d loss / d parameter}, x = d loss / dx, acts, pres) in ``dtype`` on the CPU."""
    names = param_names(sd)
    leaves = {n: sd[n].detach().to(dtype).clone().requires_grad_(True) for n in names}
    x = obs["x"].detach().to(dtype).clone().requires_grad_(True)
    B = x.shape[0]
    out = chest_ref({n: v.as_subclass(_Attached) for n, v in leaves.items()}, dict(obs, x=x), std_fixed, masks=masks, pool_idx=pool_idx,
                    dtype=dtype)
    loss = out["loss"] / B
    gs = torch.autograd.grad(loss, [x] + [leaves[n] for n in names])
    plain = lambda t: torch.Tensor.detach(t).as_subclass(torch.Tensor)
    return {"loss": plain(loss), "x": plain(gs[0]), "grads": {n: plain(g) for n, g in zip(names, gs[1:])},
            "acts": [plain(a) for a in out["acts"]], "pres": [plain(a) for a in out["pres"]]}


def dropout_masks(relu_masks, keeps, p):
    """The pinned oracle's masks of a Dropout run: the device's ReLU decisions, times keep / (1 - p) at the a1 sites.
    ``relu_masks``: 17 tensors of 0/1 (f64); ``keeps``: the eight bool tensors of ``dropout_keep``."""
    out = [m.clone() for m in relu_masks]
    for k, site in enumerate(A1_SITES):
        out[site] = out[site] * keeps[k].to(out[site].dtype) / (1.0 - p)
    return out


def tail_ref(b0, t0, clip_coef, hp):
    """f64 AdamW + EMA of one step (tests/test_gpu_optim.py's ``ref_update`` with the EMA's start as a parameter): ``b0`` = dict of
    flat p, g, m, v, ema before the step, ``t0`` successful steps so far, ``hp`` with lr, betas, wd, eps, ema_rate,
    lr_warmup_steps, ema_update_after.  Returns {name: (value, element-wise bound)}."""
    p0, g, m0, v0, e0 = (b0[k].double() for k in ("p", "g", "m", "v", "ema"))
    lr = hp.lr * train_ref.linear_warmup(hp.lr_warmup_steps)(t0)
    b1, b2 = hp.betas
    t = t0 + 1
    gc = g * clip_coef
    m = m0 + (gc - m0) * (1 - b1)
    v = v0 * b2 + (1 - b2) * gc * gc
    denom = v.sqrt() / math.sqrt(1 - b2 ** t) + hp.eps
    step = lr / (1 - b1 ** t)
    upd = step * m / denom
    p = p0 * (1 - lr * hp.wd) - upd
    d = train_ref.ema_decay(t0, hp.ema_rate, hp.ema_update_after)
    ema = p.clone() if d is None else e0 - (e0 - p) * (1.0 - d)
    tol_m = 8 * U * (m0.abs() + gc.abs())
    tol_upd = 128 * U * upd.abs() + step * tol_m / denom
    tol_p = 8 * U * (p0.abs() + upd.abs()) + tol_upd
    tol_e = tol_p if d is None else tol_p + 8 * U * (e0.abs() + p.abs())
    return {"p": (p, tol_p), "m": (m, tol_m), "v": (v, 8 * U * v), "ema": (ema, tol_e)}


def f64_loop(sd, obs, steps, lr, wd=0.1, clip=200.0, std_fixed=0.0):
    """The reference's sup_epoch on one fixed batch in f64 without Dropout: AdamW under LambdaLR(linear_warmup(1)),
    clip_grad_norm_.  Returns the mean losses before every step and after the last one."""
    names = param_names(sd)
    P = {n: sd[n].detach().double().clone().requires_grad_(True) for n in names}
    params = [P[n] for n in names]
    opt = torch.optim.AdamW(params, lr=lr, weight_decay=wd, betas=(0.9, 0.999), eps=1e-8)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, train_ref.linear_warmup(1))
    B = obs["x"].shape[0]
    mean = lambda: chest_ref({n: v.as_subclass(_Attached) for n, v in P.items()}, obs, std_fixed)["loss"].as_subclass(torch.Tensor) / B
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = mean()
        losses.append(float(loss.detach()))
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, clip)
        opt.step()
        sched.step()
    with torch.no_grad():
        losses.append(float(mean()))
    return losses
