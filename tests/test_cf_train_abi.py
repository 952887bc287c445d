"""Counterfactual fine-tuning without a GPU: the entry points of csrc/cf_train.hip (and the constant-lr AdamW) are declared, exported
and bound, bad arguments are refused before anything is launched with a message, the step tail's additions leave its defaults alone,
and ``CfTrainStep`` refuses what it does not serve before it touches a device."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest

from conftest import ROOT, load_golden

A = 4096  # a fake device address: validation must reject before any use
NEW = ("cgen_nonfinite_partial", "cgen_cf_lagrange", "cgen_lagrange_step", "cgen_adamw_ema_const_lr")


def test_symbols_declared_exported_and_bound():
    from causal_gen_amd import _lib

    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "cgen_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert hasattr(lib.cdll, name) and name in _lib.PROTOTYPES, name
    assert "typedef struct cgen_cf_lagrange_args {" in hdr and "typedef struct cgen_lagrange_step_args {" in hdr
    assert "csrc/cf_train.hip" in open(os.path.join(ROOT, "causal-gen_amd", "build.sh")).read()


def test_struct_layouts_follow_the_header():
    """Pointers first, then 4-byte fields in the header's order: the ctypes mirror has the size the C compiler gives."""
    from causal_gen_amd import _lib

    assert C.sizeof(_lib.CfLagrangeArgs) == 6 * 8 + 6 * 4 + 5 * 8
    assert _lib.CfLagrangeArgs.n_nonfinite.offset == 48 and _lib.CfLagrangeArgs.res.offset == 72
    assert C.sizeof(_lib.LagrangeStepArgs) == 6 * 8 + 6 * 4
    assert _lib.LagrangeStepArgs.lr.offset == 48 and _lib.LagrangeStepArgs.ema_update_after.offset == 68


def _lagrange(**kw):
    from causal_gen_amd import _lib

    q = _lib.CfLagrangeArgs()
    q.out3 = q.aux_sum = q.lmbda = q.nonfinite = q.res = q.coef = q.gsq_slot = q.gate = q.sums = A
    q.n_nonfinite, q.inv_b, q.eps, q.damping, q.seed_scale, q.beta = 4, 0.25, 2.0, 10.0, 1e-3, 1.0
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def _lagstep(**kw):
    from causal_gen_amd import _lib

    q = _lib.LagrangeStepArgs()
    q.lmbda = q.m = q.v = q.ema = q.g = q.state_dev = A
    q.lr, q.beta1, q.beta2, q.eps, q.ema_beta, q.ema_update_after = 1e-2, 0.9, 0.9, 1e-8, 0.999, 100
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def _refused(lib, name, args, needle):
    rc = getattr(lib, "_raw_" + name)(*args)
    assert rc < 0, name
    msg = lib.last_error().decode()
    assert name in msg and needle in msg, msg


@pytest.mark.parametrize("kw,needle", [(dict(out3=None), "out3"), (dict(aux_sum=None), "aux_sum"), (dict(lmbda=None), "lmbda"),
                                       (dict(res=None), "output"), (dict(coef=None), "output"), (dict(gsq_slot=None), "output"),
                                       (dict(gate=None), "output"), (dict(sums=None), "output"), (dict(nonfinite=None), "non-finite"),
                                       (dict(n_nonfinite=-1), "non-finite"), (dict(inv_b=0.0), "inv_b"), (dict(inv_b=2.0), "inv_b"),
                                       (dict(seed_scale=0.0), "seed_scale")])
def test_cf_lagrange_refuses_bad_arguments_before_launch(kw, needle):
    from causal_gen_amd import _lib

    lib = _lib.load()
    _refused(lib, "cgen_cf_lagrange", (C.byref(_lagrange(**kw)), None), needle)


def test_null_argument_blocks_are_refused():
    from causal_gen_amd import _lib

    lib = _lib.load()
    _refused(lib, "cgen_cf_lagrange", (None, None), "null")
    _refused(lib, "cgen_lagrange_step", (None, None), "null")
    with pytest.raises(_lib.CgenError, match="cgen_lagrange_step"):
        lib.lagrange_step(None, None)


@pytest.mark.parametrize("kw,needle", [(dict(lmbda=None), "lmbda"), (dict(m=None), "lmbda"), (dict(v=None), "lmbda"), (dict(g=None), "lmbda"),
                                       (dict(state_dev=None), "state_dev"), (dict(lr=0.0), "lr"), (dict(lr=-1e-2), "lr"),
                                       (dict(beta1=1.0), "betas"), (dict(beta2=-0.1), "betas")])
def test_lagrange_step_refuses_bad_arguments_before_launch(kw, needle):
    from causal_gen_amd import _lib

    lib = _lib.load()
    _refused(lib, "cgen_lagrange_step", (C.byref(_lagstep(**kw)), None), needle)


@pytest.mark.parametrize("what,needle", [("dtype", "dtype"), ("view", "null"), ("partial", "null"), ("n", "sizes"), ("c", "sizes"),
                                         ("nblk", "sizes"), ("stride", "channel stride"), ("big", "2^31")])
def test_nonfinite_partial_refuses_bad_arguments_before_launch(what, needle):
    from causal_gen_amd import _lib

    lib = _lib.load()
    dt, n, h, w, c, sw, p, part, nblk = _lib.F32, 2, 4, 4, 3, 8, A, A, 16
    if what == "dtype":
        dt = 7
    elif what == "view":
        p = None
    elif what == "partial":
        part = None
    elif what == "n":
        n = 0
    elif what == "c":
        c = 0
    elif what == "nblk":
        nblk = 0
    elif what == "stride":
        sw = 2
    elif what == "big":
        n, h, w = 1 << 11, 1 << 10, 1 << 10
    v = _lib.View(p, h * w * sw, w * sw, sw, c, 0)
    _refused(lib, "cgen_nonfinite_partial", (dt, n, h, w, v, part, nblk, None), needle)


def test_adamw_const_lr_takes_any_warmup_and_refuses_nulls():
    """The constant-lr entry ignores warmup_steps (0 is fine there); cgen_adamw_ema's refusal of it stands (tests/test_optim_abi.py)."""
    from causal_gen_amd import _lib

    lib = _lib.load()
    q = _lib.AdamwArgs()
    q.p = q.g = q.m = q.v = q.ema = q.state_dev = A
    q.count, q.lr, q.beta1, q.beta2, q.eps, q.wd, q.ema_beta, q.warmup_steps, q.ema_update_after = 0, 1e-3, 0.9, 0.9, 1e-8, 0.01, 0.999, 0, 100
    assert lib._raw_cgen_adamw_ema_const_lr(C.byref(q), None) == 0  # (count 0: validated, nothing launched)
    assert lib._raw_cgen_adamw_ema(C.byref(q), None) < 0
    q.p = None
    _refused(lib, "cgen_adamw_ema_const_lr", (C.byref(q), None), "bad args")


def test_step_tail_defaults_are_unchanged():
    from causal_gen_amd.step_tail import HyperParams

    hp = HyperParams(1e-3, (0.9, 0.9), 1e-8, 0.01, 350.0, 500.0, 100, 0.999, 100)  # the nine-field positional construction
    assert hp.const_lr is False and len(hp) == 10
    assert HyperParams(1e-3, (0.9, 0.9), 1e-8, 0.01, 350.0, 500.0, 1, 0.999, 100, True).const_lr is True


class _Calls:
    """Stands in for the library: records the tail's launches."""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        return lambda *a: self.log.append((name, a))


def _tail_run(extra, hook, const_lr=False):
    import torch

    from causal_gen_amd.step_tail import HyperParams, StepTail

    lib = _Calls()
    tail = StepTail(lib, 8, "cpu", 4, **({"extra_norm_slots": extra} if extra else {}))
    buf = torch.zeros(8)
    hp = HyperParams(1e-3, (0.9, 0.9), 1e-8, 0.01, 350.0, 500.0, 100, 0.999, 100, *((True,) if const_lr else ()))
    tail.run(hp, buf, buf, buf, None, 0, **({"before_commit": hook} if hook else {}))
    return tail, lib.log


def test_step_tail_launch_sequence_with_and_without_the_additions():
    tail, log = _tail_run(0, None)
    assert [n for n, _ in log] == ["sumsq_partial", "clip_decide", "adamw_ema", "step_commit"]
    assert tail.partial.numel() == 4 and log[0][1][3] == 4 and log[1][1][1] == 4
    seen = []
    tail, log = _tail_run(1, lambda stream: seen.append(stream), const_lr=True)
    assert [n for n, _ in log] == ["sumsq_partial", "clip_decide", "adamw_ema_const_lr", "step_commit"] and seen == [0]
    assert tail.partial.numel() == 5 and log[0][1][3] == 4 and log[1][1][1] == 5  # the norm's kernel writes 4, the decision sums 5
    assert tail.extra_slot(0) == tail.partial.data_ptr() + 16
    with pytest.raises(IndexError):
        tail.extra_slot(1)


def _dscm(compute_dtype="f32", **over):
    from causal_gen_amd import dscm, predictor, vae
    from causal_gen_amd.hps import Hparams

    fx = load_golden("tiny_default_c1.pt")
    hpd = dict(fx["hp"])
    m = vae.HVAE(Hparams(**hpd))
    m.compute_dtype = compute_dtype
    args = SimpleNamespace(**{**hpd, "parents_x": ["p0", "p1", "p2"], "dataset": "none", "lmbda_init": 0.8, "elbo_constraint": 2.0,
                              "damping": 10.0, **over})
    pred = predictor.make_predictor(SimpleNamespace(dataset="morphomnist", input_channels=1, input_res=16, std_fixed=0.0))
    return dscm.DSCM(args, None, pred, m), args


@pytest.mark.parametrize("what,needle", [("particles", "cf_particles"), ("f16", "16-bit fine-tuning is not validated"),
                                         ("lr_lagrange", "learning rates"), ("lr_lagrange_neg", "learning rates"), ("lr", "learning rates"),
                                         ("group", "process group"), ("head", "DGaussNet and DmolNet")])
def test_cf_train_step_refuses_before_touching_a_device(what, needle, monkeypatch):
    from causal_gen_amd import _lib
    from causal_gen_amd.cf_train import CfTrainStep

    def no_device():
        raise AssertionError("the refusal must come before any device work")

    monkeypatch.setattr(_lib, "require_gpu", no_device)
    model, args = _dscm("f16" if what == "f16" else "f32", **({"cf_particles": 2} if what == "particles" else {}))
    kw = {}
    if what == "lr_lagrange":
        kw["lr_lagrange"] = 0.0
    elif what == "lr_lagrange_neg":
        kw["lr_lagrange"] = -1e-2
    elif what == "lr":
        kw["lr"] = 0.0
    elif what == "group":
        kw["process_group"] = object()
    elif what == "head":
        model.vae.likelihood.logit_space = True
    with pytest.raises(ValueError, match=needle):
        CfTrainStep(model, args, **kw)
    assert all(not p.is_cuda for p in model.parameters())


def test_cf_train_step_is_exported_next_to_the_other_steps():
    import causal_gen_amd

    from causal_gen_amd.cf_train import CfTrainStep

    assert causal_gen_amd.CfTrainStep is CfTrainStep
