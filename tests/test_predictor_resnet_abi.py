"""ChestPredictor's entry points without a GPU: exported, declared and bound at ABI 411; every one rejects bad arguments before
any launch, with a message that names the argument; the workspace query grows with n and res."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

NAMES = ("cgen_resnet_workspace", "cgen_resnet_site", "cgen_resnet_fwd", "cgen_resnet_bwd")
FAKE = 4096  # a fake device address: validation must reject before anything dereferences it


def _args(**kw):
    from causal_gen_amd import _lib

    a = _lib.ResnetArgs()
    a.res, a.ctx, a.ctx_stride = 64, FAKE, 1
    for i in range(_lib.RESNET_CONVS):
        a.img_fwd[i] = a.img_dg[i] = a.gamma[i] = a.beta[i] = FAKE
    for h in range(4):
        a.fc_w[h] = a.fc_b[h] = a.obs[h] = FAKE
        a.obs_stride[h] = 3 if h == 1 else 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_resnet_symbols_are_exported_declared_and_bound_at_abi_411():
    from causal_gen_amd import _lib

    header = open(os.path.join(ROOT, "include", "cgen_hip.h")).read()
    assert re.search(r"#define CGEN_ABI_VERSION 411\b", header)
    lib = _lib.load()
    assert lib.version() == 411 == _lib.ABI_VERSION
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(lib.cdll, name), name
    assert _lib.RESNET_CONVS == int(re.search(r"#define CGEN_RESNET_CONVS (\d+)", header).group(1)) == 20
    assert _lib.RESNET_SITES == int(re.search(r"#define CGEN_RESNET_SITES (\d+)", header).group(1)) == 18
    # the record is laid out as the header says: 8 int32-sized fields, then 20 + 20 + 20 + 20 + 4 + 4 + 4 + 1 pointers
    assert ctypes.sizeof(_lib.ResnetArgs) == 32 + 8 * 93


def test_resnet_entry_points_reject_bad_arguments_before_any_launch():
    from causal_gen_amd import _lib

    lib = _lib.load()
    need = _lib.i64(0)
    lib.resnet_workspace(2, 64, ctypes.byref(need))
    big = need.value

    def fwd(a, n=2, x=FAKE, ws=FAKE, ws_floats=None, terms=FAKE, outs=None, loss=None):
        return lib._raw_cgen_resnet_fwd(ctypes.byref(a) if a is not None else None, n, x, ws, big if ws_floats is None else ws_floats,
                                        terms, outs, loss, None)

    def bwd(a, n=2, ws=FAKE, ws_floats=None, coef=FAKE, dx=FAKE):
        return lib._raw_cgen_resnet_bwd(ctypes.byref(a) if a is not None else None, n, ws, big if ws_floats is None else ws_floats,
                                        coef, dx, None)

    no_img, no_gamma, no_fc, no_obs = _args(), _args(), _args(), _args()
    no_img.img_dg[7] = None
    no_gamma.gamma[3] = None
    no_fc.fc_w[2] = None
    no_obs.obs[1] = None
    cases = [
        (lambda: fwd(None), "null args"),
        (lambda: fwd(_args(), n=0), "n = 0"),
        (lambda: fwd(_args(res=31)), "res = 31"),
        (lambda: fwd(_args(res=257)), "res = 257"),
        (lambda: fwd(_args(), x=None), "null x"),
        (lambda: fwd(_args(), ws=None), "ws is null"),
        (lambda: fwd(_args(), ws=FAKE + 4), "16-byte aligned"),
        (lambda: fwd(_args(), ws_floats=big - 1), "ws_floats"),
        (lambda: fwd(no_img), "weight image 7"),
        (lambda: fwd(no_gamma), "gamma / beta 3"),
        (lambda: fwd(no_fc), "fc_w / fc_b of head 2"),
        (lambda: fwd(no_obs), "obs of head 1"),
        (lambda: fwd(_args(ctx=None)), "ctx"),
        (lambda: fwd(_args(), terms=None), "nothing to write"),
        (lambda: fwd(_args(), terms=None, outs=FAKE, loss=FAKE), "loss needs terms"),
        (lambda: bwd(None), "null args"),
        (lambda: bwd(_args(), n=-1), "n = -1"),
        (lambda: bwd(_args(res=16)), "res = 16"),
        (lambda: bwd(_args(), dx=None), "null dx"),
        (lambda: bwd(_args(), ws=None), "ws is null"),
        (lambda: bwd(_args(), ws_floats=big // 2), "ws_floats"),
        (lambda: bwd(_args(), coef=None), "null coef_dev"),
        (lambda: bwd(no_obs), "obs of head 1"),
    ]
    for call, words in cases:
        assert call() < 0, words
        msg = lib.last_error().decode()
        assert words in msg and "cgen_resnet_" in msg, (words, msg)
    off, h, c = _lib.i64(0), _lib.i32(0), _lib.i32(0)
    for n, res, site, words in ((0, 64, 0, "n = 0"), (2, 300, 0, "res = 300"), (2, 64, 18, "site = 18"), (2, 64, -1, "site = -1")):
        assert lib._raw_cgen_resnet_site(n, res, site, ctypes.byref(off), ctypes.byref(h), ctypes.byref(c)) < 0
        assert words in lib.last_error().decode()
    assert lib._raw_cgen_resnet_workspace(2, 64, None) < 0 and "null floats" in lib.last_error().decode()
    assert lib._raw_cgen_resnet_workspace(0, 64, ctypes.byref(need)) < 0 and "n = 0" in lib.last_error().decode()
    assert lib._raw_cgen_resnet_workspace(2, 24, ctypes.byref(need)) < 0 and "res = 24" in lib.last_error().decode()
    with pytest.raises(_lib.CgenError, match="cgen_resnet_workspace"):
        lib.resnet_workspace(2, 1000, ctypes.byref(need))


def test_resnet_workspace_is_monotone_and_sites_lie_inside_it():
    from causal_gen_amd import _lib

    lib = _lib.load()

    def ws(n, res):
        need = _lib.i64(0)
        lib.resnet_workspace(n, res, ctypes.byref(need))
        return need.value

    for res in (32, 33, 64, 100, 192, 224, 256):
        sizes = [ws(n, res) for n in (1, 2, 3, 8, 32)]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes), res
    for n in (1, 4):
        sizes = [ws(n, res) for res in range(32, 257)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), n
        assert sizes[-1] > sizes[0]
    # the 18 activation sites: the architecture's maps, 16-byte aligned, disjoint and inside the workspace
    for n, res, maps in ((3, 33, (17, 9, 5, 3, 2)), (2, 224, (112, 56, 28, 14, 7)), (1, 32, (16, 8, 4, 2, 1))):
        total, spans = ws(n, res), []
        for site in range(_lib.RESNET_SITES):
            off, h, c = _lib.i64(0), _lib.i32(0), _lib.i32(0)
            lib.resnet_site(n, res, site, ctypes.byref(off), ctypes.byref(h), ctypes.byref(c))
            if site == 0:
                want = (maps[0], 64)
            elif site == 17:
                want = (maps[1], 64)
            else:
                stage = (site - 1) // 4
                want = (maps[1 + stage], 64 << stage)
            assert (h.value, c.value) == want, (res, site)
            assert off.value % 4 == 0 and 0 <= off.value and off.value + n * h.value * h.value * c.value <= total
            spans.append((off.value, off.value + n * h.value * h.value * c.value))
        spans.sort()
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
