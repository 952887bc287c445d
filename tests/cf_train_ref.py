"""f64 restatements of csrc/cf_train.hip for the tests (no GPU, no project code): the per-block non-finite counts, the Lagrangian of
dscm.py:78-88 with the bookkeeping of train_cf.py:161-164 / 205-210, and the multiplier's optimiser step of train_cf.py:174-177
(``AdamW(maximize=True, weight_decay=0)``, ``clamp_(min=0)``, the reference EMA with oracle/train_ref.ema_decay)."""
import math

import numpy as np

from oracle import train_ref

U = 2.0 ** -24


def nonfinite_counts(logical, nblk):
    """partial[b] for the logical (unpadded) elements in NHWC order: element i belongs to block (i // 256) % nblk."""
    flat = np.asarray(logical, dtype=np.float64).reshape(-1)
    bad = ~np.isfinite(flat)
    out = np.zeros(nblk, dtype=np.int64)
    idx = np.nonzero(bad)[0]
    np.add.at(out, (idx // 256) % nblk, 1)
    return out


def lagrange(out3, aux_sum, aux_add, B, lmbda, eps, damping, seed_scale, beta, n_nonfinite, sums):
    """Every output of cgen_cf_lagrange in f64, with `tol`: 8 u (sum of the magnitudes of the terms that form the value)."""
    elbo, nll, kl = (float(v) for v in out3)
    aux_terms = abs(aux_sum) + (abs(aux_add) if aux_add is not None else 0.0)
    aux = (aux_sum + (aux_add if aux_add is not None else 0.0)) / B
    c = eps - elbo
    w = lmbda - damping * c
    loss = aux - w * c
    g = -c
    t_c = abs(eps) + abs(elbo)
    t_w = abs(lmbda) + abs(damping) * t_c
    t_loss = aux_terms / B + t_w * t_c
    bad = (not math.isfinite(loss)) or n_nonfinite > 0
    res = {"loss": (loss, 8 * U * t_loss), "aux_loss": (aux, 8 * U * aux_terms / B), "g_lmbda": (g, 8 * U * t_c), "w": (w, 8 * U * t_w),
           "coef0": (w * seed_scale, 8 * U * t_w * seed_scale), "coef1": (w * beta * seed_scale, 8 * U * t_w * abs(beta) * seed_scale),
           "coef2": (beta, 0.0), "gsq": (g * g, 8 * U * t_c * t_c), "gate0": (loss, 8 * U * t_loss),
           "gate1": (float("nan") if bad else nll, 0.0), "gate2": (kl, 0.0)}
    new = list(sums)
    if bad:
        new[6] += 1.0
    else:
        for i, v in enumerate((loss, aux, elbo, nll, kl, 1.0)):
            new[i] += v
    tol_sums = [8 * U * (abs(s) + t) for s, t in zip(sums, (t_loss, aux_terms / B, abs(elbo), abs(nll), abs(kl), 1.0, 1.0, 0.0))]
    return res, bad, new, tol_sums


def lagrange_step(lmbda, m, v, ema, g_lmbda, clip, t0, lr, betas, eps, ema_beta, ema_after):
    """One successful step after t0 successful ones.  Returns {name: (value, tol)} with the one-element bounds of
    tests/test_gpu_optim.py (m 8u, v 8u, update 128u, p 8u, ema 8u) -- the clamp adds nothing: max(p, 0) moves p towards the reference
    or onto it."""
    b1, b2 = betas
    t = t0 + 1
    g = -(g_lmbda * clip)
    m1 = m + (g - m) * (1 - b1)
    v1 = v * b2 + (1 - b2) * g * g
    denom = math.sqrt(v1) / math.sqrt(1 - b2 ** t) + eps
    step = lr / (1 - b1 ** t)
    upd = step * m1 / denom
    p = max(lmbda - upd, 0.0)
    d = train_ref.ema_decay(t0, ema_beta, ema_after)
    e = p if d is None else ema - (ema - p) * (1.0 - d)
    tol_m = 8 * U * (abs(m) + abs(g))
    tol_upd = 128 * U * abs(upd) + step * tol_m / denom
    tol_p = 8 * U * (abs(lmbda) + abs(upd)) + tol_upd
    tol_e = tol_p if d is None else tol_p + 8 * U * (abs(ema) + abs(p))
    return {"lmbda": (p, tol_p), "m": (m1, tol_m), "v": (v1, 8 * U * v1), "ema": (e, tol_e)}
