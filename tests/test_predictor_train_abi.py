"""Training of the anticausal predictors without a GPU: the three entry points are exported, declared and bound at ABI 411, four
head records fit the kernel-argument segment, every entry rejects bad arguments before anything is launched with a message naming
the cause, the workspace query follows the stack geometry, and the training kernels of the gfx950 code object use no scratch."""
import ctypes as C
import os
import re

import pytest

import codeobj
from conftest import ROOT

ENTRIES = ("cgen_predictor_train_workspace", "cgen_predictor_train_fwd", "cgen_predictor_train_bwd")
X, WS, T, DX, COEF = 8192, 12288, 16384, 20480, 24576  # fake device addresses: validation must reject before dereferencing any


def _rec(**kw):
    from causal_gen_amd import _lib

    r = _lib.PredTrainHead()
    h = r.hd
    h.c, h.res, h.width, h.nout, h.ctx, h.kind, h.obs_stride = 1, 32, 8, 2, 0, _lib.PRED_NORMAL, 1
    for i in range(8):
        h.w[i], r.gw[i] = 4096, 4096
    h.b[7], h.obs, r.gb = 4096, 4096, 4096
    for i in range(7):
        for f in ("gamma", "beta", "running_mean", "running_var", "num_batches_tracked", "ggamma", "gbeta"):
            getattr(r, f)[i] = 4096
    for k, v in kw.items():
        setattr(r.hd if hasattr(r.hd, k) else r, k, v)
    return r


def _recs(*recs):
    from causal_gen_amd import _lib

    return (_lib.PredTrainHead * len(recs))(*recs)


def test_symbols_exported_declared_and_bound_at_abi_411():
    from causal_gen_amd import _lib

    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "cgen_hip.h")).read()
    assert "#define CGEN_ABI_VERSION 411" in hdr and lib.version() == 411 == _lib.ABI_VERSION
    for name in ENTRIES:
        assert re.search(r"\bint %s\(const cgen_pred_train_head\* heads," % name, hdr), name
        assert hasattr(lib.cdll, name) and name in _lib.PROTOTYPES, name
    assert "typedef struct cgen_pred_train_head {" in hdr


def test_head_records_fit_the_kernel_argument_segment():
    """(the record's layout against the header: tests/test_abi_mirror.py)"""
    from causal_gen_amd import _lib

    assert C.sizeof(_lib.PredTrainHead) * _lib.PRED_MAX_HEADS < 3500  # four records travel by value in a 4 KiB kernel-argument segment


def _stack_floats(res, width):
    s1 = 2 if res > 64 else 1
    h1 = (res - 1) // s1 + 1
    pool = res > 32
    p = h1 // 2 if pool else h1
    h2 = (p - 1) // 2 + 1
    h4 = (h2 - 1) // 2 + 1
    h6 = (h4 - 1) // 2 + 1
    w = width
    total = w * h1 * h1 + (w * p * p if pool else 0) + 2 * (2 * w * h2 * h2) + 2 * (4 * w * h4 * h4) + 8 * w * h6 * h6
    return (total + 3) // 4 * 4, (h1, h2, h2, h4, h4, h6)


def _want_workspace(c, res, w, nheads, n):
    """two stacks per (image, head), mean and 1/std of 29 w BatchNorm channels per head, the tail's rows (features + 4, fc.0 output,
    hidden, its gradient, 16 outputs per image) and the partial sums of the most-split weight gradient (4096 pixels per slice, 64 at the most)"""
    stack, hs = _stack_floats(res, w)
    chans = [(c, w, 49), (w, 2 * w, 9), (2 * w, 2 * w, 9), (2 * w, 4 * w, 9), (4 * w, 4 * w, 9), (4 * w, 8 * w, 9)]
    part = 0
    for (ci, co, k), h in zip(chans, hs):
        tot = n * h * h
        ns = min(64, -(-tot // 4096))
        chunk = -(-tot // ns)
        ns = -(-tot // chunk)
        part = max(part, ns * ci * co * k if ns > 1 else 0)
    tail = (n * (8 * w + 4 + 24 * w + 16) + 3) // 4 * 4
    return 2 * n * nheads * stack + nheads * 58 * w + nheads * (tail + (part + 3) // 4 * 4)


def test_workspace_follows_the_geometry():
    from causal_gen_amd import _lib

    lib = _lib.load()
    for c, res, w in [(1, 192, 16), (1, 32, 8), (3, 40, 8), (1, 9, 16), (1, 66, 32), (1, 72, 24)]:
        for nheads, n in ((1, 2), (3, 5), (4, 32)):
            recs = _recs(*[_rec(c=c, res=res, width=w) for _ in range(nheads)])
            got = _lib.i64(0)
            lib.predictor_train_workspace(recs, nheads, n, C.byref(got))
            assert got.value == _want_workspace(c, res, w, nheads, n), (c, res, w, nheads, n)
    for recs, nh, n, words in [(_recs(_rec(width=8), _rec(width=16)), 2, 2, "does not take these heads"),
                               (_recs(_rec(res=4)), 1, 2, "does not take these heads"), (_recs(_rec()), 1, 1, "at least 2 images"),
                               (None, 1, 2, "does not take these heads")]:
        with pytest.raises(_lib.CgenError, match=words):
            lib.predictor_train_workspace(recs, nh, n, C.byref(_lib.i64(0)))
    with pytest.raises(_lib.CgenError, match="null output"):
        lib.predictor_train_workspace(_recs(_rec()), 1, 2, None)


def test_entry_points_reject_bad_arguments_before_launch():
    from causal_gen_amd import _lib

    lib = _lib.load()

    def both(recs, nh, n, ws=WS, ws_floats=1 << 40, x=X):
        out = []
        rc = lib._raw_cgen_predictor_train_fwd(recs, nh, n, x, ws, ws_floats, 0.1, T, None, None, None)
        out.append((rc, lib.last_error().decode()))
        rc = lib._raw_cgen_predictor_train_bwd(recs, nh, n, x, ws, ws_floats, COEF, DX, None)
        out.append((rc, lib.last_error().decode()))
        return out

    good = _recs(_rec(res=66, width=16))
    need = _lib.i64(0)
    lib.predictor_train_workspace(good, 1, 4, C.byref(need))
    null = lambda field, i: (lambda r: getattr(r, field).__setitem__(i, None))
    cases = [
        (both(good, 1, 4, ws=None), "null workspace"),
        (both(good, 1, 4, ws_floats=need.value - 1), "workspace too small"),
        (both(good, 1, 4, x=None), "null image"),
        (both(good, 1, 1), "at least 2 images"),
        (both(None, 1, 4), "head records"),
        (both(good, 5, 4), "head records"),
        (both(_recs(_rec(width=8), _rec(width=16)), 2, 4), "equal widths"),
        (both(_recs(_rec(res=4)), 1, 4), "unsupported input shape"),
        (both(_recs(_rec(res=600)), 1, 4), "unsupported input shape"),
        (both(_recs(_rec(c=5)), 1, 4), "unsupported input shape"),
        (both(_recs(_rec(width=12)), 1, 4), "unsupported width"),
        (both(_recs(_rec(kind=7)), 1, 4), "unknown variable kind"),
        (both(_recs(_rec(nout=3)), 1, 4), "do not fit variable kind"),
        (both(_recs(_rec(ctx=1)), 1, 4), "context mismatch"),
        (both(_recs(_rec(obs=None)), 1, 4), "null obs"),
        (both(_recs(_rec(gb=None)), 1, 4), "fc.3's bias"),
    ]
    for field, i, words in [("gamma", 2, "null BatchNorm pointer"), ("running_var", 6, "null BatchNorm pointer"),
                            ("num_batches_tracked", 0, "null BatchNorm pointer"), ("gbeta", 3, "null BatchNorm gradient pointer"),
                            ("gw", 5, "null weight gradient pointer")]:
        r = _rec()
        null(field, i)(r)
        cases.append((both(_recs(r), 1, 4), words))
    r = _rec()
    r.hd.w[3] = None
    cases.append((both(_recs(r), 1, 4), "null weight pointer"))
    r = _rec()
    r.hd.b[7] = None
    cases.append((both(_recs(r), 1, 4), "null weight pointer"))
    for res, words in cases:
        for rc, msg in res:
            assert rc < 0 and words in msg, (words, msg)
    one = _recs(_rec())
    rc = lib._raw_cgen_predictor_train_fwd(one, 1, 4, X, WS, 1 << 40, 0.1, None, None, None, None)
    assert rc < 0 and "null terms" in lib.last_error().decode()
    rc = lib._raw_cgen_predictor_train_fwd(one, 1, 4, X, WS, 1 << 40, 1.5, T, None, None, None)
    assert rc < 0 and "momentum" in lib.last_error().decode()
    with pytest.raises(_lib.CgenError, match="null coef_dev"):
        lib.predictor_train_bwd(one, 1, 4, X, WS, 1 << 40, None, DX, None)


def test_python_step_rejects_bad_setups_before_any_device_work():
    """(no GPU: the class refuses to start; the argument checks of its constructor come first)"""
    from causal_gen_amd import predictor_train as PT

    with pytest.raises(ValueError, match="lr_warmup_steps"):
        PT.PredictorTrainStep(None, lr_warmup_steps=0)
    assert PT.BN_MOMENTUM == 0.1


def test_training_kernels_have_no_scratch_and_no_spills():
    seen = {}
    for name, scratch, spills in codeobj.kernels():
        k = re.search(r"\d+(ptrain_[a-z0-9_]+?)(?:I|E)", name)
        if not k:
            continue
        seen[k.group(1)] = seen.get(k.group(1), 0) + 1
        assert scratch == 0, (name, scratch)
        assert spills == 0, (name, spills)
    # the 7x7 and the 3x3 form of the forward conv and of the weight gradient, the forward and backward form of the tail's output
    # stage; one of everything else
    assert seen == {"ptrain_conv_fwd": 2, "ptrain_bn_fwd": 1, "ptrain_tail_fc0": 1, "ptrain_tail_bn": 1, "ptrain_tail_out": 2,
                    "ptrain_tail_bn_bwd": 1, "ptrain_tail_fc_wgrad": 1, "ptrain_tail_fc0_dgrad": 1, "ptrain_bn_bwd": 1,
                    "ptrain_conv_wgrad": 2, "ptrain_wgrad_reduce": 1}, seen
