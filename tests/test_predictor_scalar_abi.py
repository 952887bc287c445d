"""The train-mode scalar head (cgen_mlp_train_*) and the planar augment entry without a GPU: the symbols are exported, declared and
bound at ABI 411, every entry rejects bad arguments before anything is launched with a message that names the cause, the
workspace query equals the header's formula, the new kernels of the gfx950 code object use no scratch, and the Python step still
checks its warm-up before it asks for a GPU.  (The record's layout against the header: tests/test_abi_mirror.py.)"""
import ctypes as C
import os
import re

import pytest

import codeobj
from conftest import ROOT

MLP_ENTRIES = ("cgen_mlp_train_workspace", "cgen_mlp_train_fwd", "cgen_mlp_train_bwd")
P, WS, T, L, COEF = 4096, 12288, 16384, 20480, 24576  # fake device addresses: validation must reject before dereferencing any


def _rec(nin=2, width=32, **kw):
    from causal_gen_amd import _lib

    r = _lib.MlpTrainHead()
    r.nin, r.width, r.obs_stride, r.obs, r.bias, r.gb = nin, width, 1, P, P, P
    for k in range(max(0, min(nin, 8))):
        r.in_[k], r.in_stride[k] = P, 1
    for i in range(3):
        r.w[i], r.gw[i] = P, P
    for i in range(2):
        for f in ("gamma", "beta", "running_mean", "running_var", "num_batches_tracked", "ggamma", "gbeta"):
            getattr(r, f)[i] = P
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_symbols_exported_declared_and_bound_at_abi_411():
    from causal_gen_amd import _lib

    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "cgen_hip.h")).read()
    assert "#define CGEN_ABI_VERSION 411" in hdr and lib.version() == 411 == _lib.ABI_VERSION
    for name in MLP_ENTRIES:
        assert re.search(r"\bint %s\(const cgen_mlp_train_head\* rec, int32_t n," % name, hdr), name
        assert hasattr(lib.cdll, name) and name in _lib.PROTOTYPES, name
    assert "typedef struct cgen_mlp_train_head {" in hdr
    assert re.search(r"\bint cgen_batch_augment_planar\(const cgen_augment_args\* a, cgen_stream_t stream\);", hdr)
    assert hasattr(lib.cdll, "cgen_batch_augment_planar") and "cgen_batch_augment_planar" in _lib.PROTOTYPES
    assert (_lib.MLP_MAX_IN, _lib.MLP_MAX_WIDTH) == (8, 64) and "#define CGEN_MLP_MAX_IN 8" in hdr and "#define CGEN_MLP_MAX_WIDTH 64" in hdr


def test_workspace_query_is_the_formula_of_the_header():
    from causal_gen_amd import _lib

    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "cgen_hip.h")).read()
    assert "/* floats of workspace for n rows: 3 * n * width + 2 * n + 2 * width */" in hdr
    for n in (2, 5, 4096):
        for w in (8, 32, 64):
            got = _lib.i64(0)
            lib.mlp_train_workspace(C.byref(_rec(width=w)), n, C.byref(got))
            assert got.value == 3 * n * w + 2 * n + 2 * w, (n, w)
    for rec, n, out, words in [(_rec(), 1, _lib.i64(0), "outside 2..4096"), (_rec(), 4097, _lib.i64(0), "outside 2..4096"),
                               (_rec(width=12), 4, _lib.i64(0), "unsupported width 12"), (_rec(width=72), 4, _lib.i64(0), "unsupported width 72"),
                               (None, 4, _lib.i64(0), "null head record"), (_rec(), 4, None, "null output")]:
        with pytest.raises(_lib.CgenError, match=words):
            lib.mlp_train_workspace(None if rec is None else C.byref(rec), n, None if out is None else C.byref(out))


def test_mlp_entries_reject_bad_arguments_before_launch():
    from causal_gen_amd import _lib

    lib = _lib.load()

    def both(rec, n, ws=WS, ws_floats=1 << 40):
        r = None if rec is None else C.byref(rec)
        out = []
        rc = lib._raw_cgen_mlp_train_fwd(r, n, ws, ws_floats, 0.1, T, L, None)
        out.append((rc, lib.last_error().decode()))
        rc = lib._raw_cgen_mlp_train_bwd(r, n, ws, ws_floats, COEF, None)
        out.append((rc, lib.last_error().decode()))
        return out

    need = 3 * 4 * 32 + 2 * 4 + 2 * 32
    cases = [
        (both(_rec(), 4, ws=None), "null workspace"),
        (both(_rec(), 4, ws_floats=need - 1), "workspace too small"),
        (both(_rec(), 1), "at least 2 rows"),
        (both(_rec(), 4097), "at most 4096 rows"),
        (both(None, 4), "null head record"),
        (both(_rec(nin=0), 4), "unsupported number of inputs 0"),
        (both(_rec(nin=9), 4), "unsupported number of inputs 9"),
        (both(_rec(width=12), 4), "unsupported width 12"),
        (both(_rec(width=72), 4), "unsupported width 72"),
        (both(_rec(obs=None), 4), "null obs"),
        (both(_rec(bias=None), 4), "null weight pointer"),
        (both(_rec(gb=None), 4), "mlp.6's bias"),
    ]
    nulls = [("in_", i, "null input column %d" % i) for i in range(2)]
    nulls += [("w", i, "null weight pointer") for i in range(3)] + [("gw", i, "null weight gradient pointer") for i in range(3)]
    for i in range(2):
        nulls += [(f, i, "null BatchNorm pointer (BatchNorm %d)" % i) for f in ("gamma", "beta", "running_mean", "running_var", "num_batches_tracked")]
        nulls += [(f, i, "null BatchNorm gradient pointer (BatchNorm %d)" % i) for f in ("ggamma", "gbeta")]
    for field, i, words in nulls:
        r = _rec()
        getattr(r, field)[i] = None
        cases.append((both(r, 4), words))
    for res, words in cases:
        for rc, msg in res:
            assert rc < 0 and words in msg, (words, msg)
    # the good record with an exact workspace passes every check of the backward up to coef_dev, of the forward up to terms / momentum
    good = C.byref(_rec())
    rc = lib._raw_cgen_mlp_train_fwd(good, 4, WS, need, 0.1, None, L, None)
    assert rc < 0 and "null terms" in lib.last_error().decode()
    for mo in (-0.1, 1.5, float("nan")):
        rc = lib._raw_cgen_mlp_train_fwd(good, 4, WS, need, mo, T, L, None)
        assert rc < 0 and "momentum" in lib.last_error().decode(), mo
    with pytest.raises(_lib.CgenError, match="null coef_dev"):
        lib.mlp_train_bwd(good, 4, WS, need, None, None)


def test_planar_augment_rejects_bad_arguments_before_launch():
    from causal_gen_amd import _lib

    lib = _lib.load()
    V = _lib.View

    def args(**kw):
        a = _lib.AugmentArgs()
        a.dtype, a.n, a.c, a.h0, a.w0, a.r_h, a.r_w, a.pad_x, a.pad_y, a.ctx = _lib.F32, 2, 3, 28, 28, 32, 32, 4, 4, 0
        a.stream_id, a.hflip_p, a.sub, a.mul, a.n_data = _lib.STREAM_AUGMENT, 0.5, 127.5, 1 / 127.5, 10
        a.data, a.index, a.rng = 4096, 8192, 12288
        a.out = V(16384, 3 * 32 * 32, 32, 1, 3, 0)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    cases = [
        (args(c=5, out=V(16384, 5 * 1024, 32, 1, 5, 0)), "c must be 1..4"),
        (args(r_h=37, out=V(16384, 3 * 37 * 32, 32, 1, 3, 0)), "larger than the padded image"),
        (args(r_w=37, out=V(16384, 3 * 32 * 37, 37, 1, 3, 0)), "larger than the padded image"),
        (args(dtype=_lib.F16), "planar output is f32"),
        (args(out=V(16384, 3 * 1024, 3 * 32, 3, 3, 0)), "contiguous [n, c, r_h, r_w]"),
        (args(out=V(None, 3 * 1024, 32, 1, 3, 0)), "null data, index or out"),
        (args(rng=None), "neither a Philox state nor injected draws"),
        (None, "null args"),
    ]
    for a, words in cases:
        assert lib._raw_cgen_batch_augment_planar(None if a is None else C.byref(a), None) < 0, words
        msg = lib.last_error().decode()
        assert words in msg, (words, msg)


def test_python_step_rejects_the_warm_up_first():
    """(no GPU: the class refuses to start; the argument checks of its constructor come first)"""
    from causal_gen_amd import predictor_train as PT

    with pytest.raises(ValueError, match="lr_warmup_steps"):
        PT.PredictorTrainStep(None, scalar_heads=True, lr_warmup_steps=0)


def test_new_kernels_have_no_scratch_and_no_spills():
    seen = {}
    for name, scratch, spills in codeobj.kernels():
        k = re.search(r"\d+(pmlp_[a-z0-9_]+?)E", name)
        if k:
            key = k.group(1)
        elif re.search(r"batch_augment_kernelI\w+Li3EE", name):  # the AUG_PLANAR instance of the augment kernel
            key = "batch_augment_kernel<planar>"
        else:
            continue
        seen[key] = seen.get(key, 0) + 1
        assert scratch == 0, (name, scratch)
        assert spills == 0, (name, spills)
    assert seen == {"pmlp_fwd": 1, "pmlp_bwd": 1, "batch_augment_kernel<planar>": 1}, seen
