"""The optimiser tail without a GPU: a warm-up of 0 steps is refused before any launch (LambdaLR(linear_warmup) divides by it;
the kernel used to compute lr = 0/0 on the first step and turn every weight, moment and EMA entry into NaN without an error)."""
import ctypes as C
import types

import pytest


def _args(warmup):
    from causal_gen_amd import _lib

    q = _lib.AdamwArgs()
    q.p = q.g = q.m = q.v = q.ema = q.state_dev = 4096  # a fake device address: validation must reject before any use
    q.count, q.lr, q.beta1, q.beta2, q.eps, q.wd, q.ema_beta = 1000, 1e-3, 0.9, 0.9, 1e-8, 0.01, 0.999
    q.warmup_steps, q.ema_update_after = warmup, 100
    return q


@pytest.mark.parametrize("warmup", [0, -1])
def test_adamw_ema_rejects_warmup_0_lr_nan_on_first_step(warmup):
    from causal_gen_amd import _lib

    lib = _lib.load()
    rc = lib._raw_cgen_adamw_ema(C.byref(_args(warmup)), None)
    assert rc < 0
    assert "warmup_steps must be > 0" in lib.last_error().decode()
    with pytest.raises(_lib.CgenError, match="cgen_adamw_ema"):
        lib.adamw_ema(C.byref(_args(warmup)), None)


@pytest.mark.parametrize("warmup", [0, -5])
def test_trainstep_rejects_lr_warmup_steps_0_before_device_work(warmup):
    from causal_gen_amd.train import TrainStep

    # no model and no GPU are needed: the check comes first
    with pytest.raises(ValueError, match="lr_warmup_steps"):
        TrainStep(None, types.SimpleNamespace(lr_warmup_steps=warmup))
