"""The tiled placement of the anticausal predictors without a GPU: support and workspace queries against a restatement of the
stack geometry, argument validation before any launch, and a gfx950 code object whose new kernels use no scratch."""
import ctypes
import re

import pytest

import codeobj

SHAPES = [(1, 192, 16), (1, 32, 8), (3, 40, 8), (1, 8, 8), (1, 66, 32)]  # (c, res, width)


def _rec(**kw):
    from causal_gen_amd import _lib

    r = _lib.PredHead()
    r.c, r.res, r.width, r.nout, r.ctx, r.kind, r.obs_stride = 1, 32, 8, 2, 0, _lib.PRED_NORMAL, 1
    for i in range(8):
        r.w[i], r.b[i] = 4096, 4096  # fake device addresses: validation must reject before anything dereferences them
    r.obs = 4096
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _recs(*recs):
    from causal_gen_amd import _lib

    return (_lib.PredHead * len(recs))(*recs)


def _stack_floats(res, width):
    """Floats of one head's activation stack: 7x7 stem (stride 2 above 64), 2x2 pool above 32, five 3x3 convs of which three
    halve; every plane kept, the whole rounded up to a multiple of 4 floats (16 bytes)."""
    s1 = 2 if res > 64 else 1
    h1 = (res - 1) // s1 + 1
    pool = res > 32
    p = h1 // 2 if pool else h1
    h2 = (p - 1) // 2 + 1
    h4 = (h2 - 1) // 2 + 1
    h6 = (h4 - 1) // 2 + 1
    w = width
    total = w * h1 * h1 + (w * p * p if pool else 0) + 2 * (2 * w * h2 * h2) + 2 * (4 * w * h4 * h4) + 8 * w * h6 * h6
    return (total + 3) // 4 * 4


def test_tiled_supported_and_workspace_match_the_stack_geometry():
    from causal_gen_amd import _lib

    lib = _lib.load()
    for c, res, w in SHAPES:
        for nheads in (1, 3):
            recs = _recs(*[_rec(c=c, res=res, width=w) for _ in range(nheads)])
            assert lib._raw_cgen_predictor_tiled_supported(recs, nheads) == 1, (c, res, w)
            for n in (1, 3):
                got = _lib.i64(0)
                lib.predictor_tiled_workspace(recs, nheads, n, ctypes.byref(got))
                assert got.value == n * nheads * _stack_floats(res, w), (c, res, w, nheads, n)
    assert _stack_floats(192, 16) * 4 * 32 * 4 == pytest.approx(125e6, rel=0.05)  # ukbb192, 4 heads, B = 32: about 125 MB
    mixed = _recs(_rec(width=8), _rec(width=16))
    assert lib._raw_cgen_predictor_tiled_supported(mixed, 2) == 0
    assert lib._raw_cgen_predictor_tiled_supported(_recs(_rec(res=4)), 1) == 0
    assert lib._raw_cgen_predictor_tiled_supported(None, 1) == 0
    with pytest.raises(_lib.CgenError, match="does not take these heads"):
        lib.predictor_tiled_workspace(mixed, 2, 1, ctypes.byref(_lib.i64(0)))


def test_tiled_entry_points_reject_bad_arguments_before_launch():
    from causal_gen_amd import _lib

    lib = _lib.load()
    X, WS, T, DX, COEF = 8192, 12288, 16384, 20480, 24576  # fake device addresses

    def need(recs, nh, n):
        v = _lib.i64(0)
        lib.predictor_tiled_workspace(recs, nh, n, ctypes.byref(v))
        return v.value

    def both(recs, nh, n, ws, ws_floats):
        """(rc, message) of the forward and of the backward entry"""
        out = []
        rc = lib._raw_cgen_predictor_tiled_fwd(recs, nh, n, X, ws, ws_floats, T, None, None, None)
        out.append((rc, lib.last_error().decode()))
        rc = lib._raw_cgen_predictor_tiled_bwd(recs, nh, n, X, ws, ws_floats, COEF, DX, None)
        out.append((rc, lib.last_error().decode()))
        return out

    good = _recs(_rec(res=192, width=16))
    full = need(good, 1, 2)
    for rc, msg in both(good, 1, 2, None, full):
        assert rc < 0 and "null workspace" in msg, msg
    for rc, msg in both(good, 1, 2, WS, full - 1):
        assert rc < 0 and "workspace too small" in msg, msg
    mixed = _recs(_rec(width=8), _rec(width=16))
    for rc, msg in both(mixed, 2, 2, WS, 1 << 40):
        assert rc < 0 and "equal widths" in msg, msg
    bad_w = _rec()
    bad_w.w[3] = None
    cases = [
        (_rec(kind=7), "unknown variable kind"),
        (bad_w, "null weight pointer"),
        (_rec(ctx=1), "context mismatch"),
        (_rec(y=4096), "context mismatch"),
        (_rec(width=12), "unsupported width"),
        (_rec(nout=3), "do not fit variable kind"),
        (_rec(res=4), "unsupported input shape"),
    ]
    for rec, words in cases:
        for rc, msg in both(_recs(rec), 1, 2, WS, 1 << 40):
            assert rc < 0 and words in msg, (words, msg)
    one = _recs(_rec())
    rc = lib._raw_cgen_predictor_tiled_fwd(one, 1, 2, X, WS, 1 << 40, None, None, None, None)
    assert rc < 0 and "nothing to write" in lib.last_error().decode()
    with pytest.raises(_lib.CgenError, match="cgen_predictor_tiled_bwd"):
        lib.predictor_tiled_bwd(one, 1, 2, X, WS, 1 << 40, None, DX, None)


def test_tiled_kernels_have_no_scratch_and_no_spills():
    seen = {}
    for name, scratch, spills in codeobj.kernels():
        k = re.search(r"(ptile_conv_fwd|ptile_conv_bwd|ptile_stem_bwd|ptile_tail)", name)
        if not k:
            continue
        seen[k.group(1)] = seen.get(k.group(1), 0) + 1
        assert scratch == 0, (name, scratch)
        assert spills == 0, (name, spills)
    # stem 2 strides x 4 channel blockings; 3x3 forward (stride 1, stride 2, stride 2 + pool) x 2 tile sizes x 4; 3x3 data
    # gradient 3 x 4; stem data gradient per stride; tail forward / backward
    assert seen == {"ptile_conv_fwd": 8 + 24, "ptile_conv_bwd": 12, "ptile_stem_bwd": 2, "ptile_tail": 2}, seen
