"""cgen_pgm_counterfactual without a GPU: exported, declared and bound at ABI 411, records and arguments fit the kernel-argument
segment, and every bad argument is rejected before anything is launched with a message naming the field."""
import ctypes as C
import os
import re

from conftest import ROOT

OBS, DO, CF, EPS, PA, CFPA, U, P, MASK = 8192, 12288, 16384, 20480, 24576, 28672, 32768, 4096, 36864  # fake device addresses


def _mech(kind, **kw):
    from causal_gen_amd import _lib

    r = _lib.PgmMech()
    r.kind, r.col, r.ncls, r.nctx, r.nhidden, r.act, r.bins, r.bound = kind, 0, 2, 1, 1, 0, 4, 3.0
    r.width[0] = 8
    for i in range(8):
        r.p[i] = P
    for k, v in kw.items():
        if isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                getattr(r, k)[i] = x
        else:
            setattr(r, k, v)
    return r


def _recs(*recs):
    from causal_gen_amd import _lib

    return (_lib.PgmMech * len(recs))(*recs)


def _args(pre=(), uniforms=(), **kw):
    from causal_gen_amd import _lib

    a = _lib.PgmCfArgs()
    a.obs, a.table_rows, a.do_table, a.do_rows, a.cf, a.ncol, a.rows = OBS, 8, DO, 8, CF, 4, 8
    for i, u in enumerate(uniforms):
        a.uniforms[i] = u
    a.npre = len(pre)
    for r, p in zip(a.pre, pre):
        r.col, r.width, r.kind, r.hi, r.lo, r.mu, r.sd = p
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_symbol_exported_declared_and_bound_at_abi_411():
    from causal_gen_amd import _lib

    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "cgen_hip.h")).read()
    assert "#define CGEN_ABI_VERSION 411" in hdr and lib.version() == 411 == _lib.ABI_VERSION
    assert re.search(r"\bint cgen_pgm_counterfactual\(const cgen_pgm_mech\* mechs, int32_t n, const cgen_pgm_cf_args\* a, cgen_stream_t\);", hdr)
    assert hasattr(lib.cdll, "cgen_pgm_counterfactual") and "cgen_pgm_counterfactual" in _lib.PROTOTYPES
    assert "typedef struct cgen_pgm_cf_args {" in hdr and "typedef struct cgen_pgm_pre {" in hdr
    assert hasattr(lib, "pgm_counterfactual")


def test_records_and_arguments_fit_the_kernel_argument_segment():
    """(the two structs' layouts and the constants against the header: tests/test_abi_mirror.py)"""
    from causal_gen_amd import _lib

    # records, arguments and the context map travel by value: the kernel-argument segment stays under 4 KiB
    assert C.sizeof(_lib.PgmMech) * _lib.PGM_MAX_MECH + C.sizeof(_lib.PgmCfArgs) + 8 * _lib.PGM_MAX_MECH + 64 < 4096


def test_bad_arguments_are_rejected_before_launch():
    from causal_gen_amd import _lib

    lib, L = _lib.load(), _lib

    def call(recs, n, a):
        rc = lib._raw_cgen_pgm_counterfactual(recs, n, None if a is None else C.byref(a), None)
        return rc, lib.last_error().decode()

    root = lambda col: _mech(L.PGM_BERNOULLI, col=col)
    aff = lambda **kw: _mech(L.PGM_AFFINE, **{**dict(col=2, nctx=2, ctx_col=[0, 1], nhidden=2, width=[32, 32]), **kw})
    gum = _mech(L.PGM_GUMBEL_MAX, col=2, ncls=2, nctx=1, ctx_col=[0], nhidden=2, width=[8, 16], act=L.PGM_SIGMOID)
    flow = _recs(root(0), root(1), aff())
    copy1 = (0, 1, L.PGM_PRE_COPY, 0.0, 0.0, 0.0, 1.0)
    cases = [
        (call(flow, 3, None), "null arguments"),
        (call(flow, 3, _args(obs=None)), "null obs"),
        (call(flow, 3, _args(cf=None)), "null cf"),
        (call(flow, 3, _args(do_table=None, do_mask=4)), "null do_table"),
        (call(flow, 3, _args(do_table=None, do_mask_dev=MASK)), "null do_table"),
        (call(flow, 3, _args(do_mask=8)), "do_mask = 0x8 has a bit at or above n = 3"),
        (call(flow, 3, _args(do_mask=1, do_rows=7)), "do_rows = 7"),
        (call(_recs(root(0), aff(), root(1)), 3, _args()), "mechanism 1: ctx_col[1] = 1 is not the col of an earlier record"),
        (call(_recs(root(0), root(1), aff(ctx_col=[0, 3])), 3, _args()), "ctx_col[1] = 3 is not the col of an earlier record"),
        (call(_recs(aff(ctx_col=[2, 2])), 1, _args()), "mechanism 0: ctx_col[0] = 2 is not the col of an earlier record"),
        (call(_recs(root(0), gum), 2, _args()), "null uniforms[1]"),
        (call(_recs(root(0), gum), 2, _args(uniforms=[U, 0])), "null uniforms[1]"),
        (call(_recs(root(0), gum), 2, _args(uniforms=[0, U], exact_gumbel=2)), "exact_gumbel = 2"),
        (call(flow, 3, _args(npre=9)), "npre = 9"),
        (call(flow, 3, _args(npre=-1)), "npre = -1"),
        (call(flow, 3, _args(pa=PA)), "npre = 0 with a parents output"),
        (call(flow, 3, _args(pre=[copy1, (3, 2, L.PGM_PRE_COPY, 0.0, 0.0, 0.0, 1.0)], pa=PA)), "pre[1]: col = 3 (+2) is out of range (ncol = 4)"),
        (call(flow, 3, _args(pre=[(-1, 1, L.PGM_PRE_COPY, 0.0, 0.0, 0.0, 1.0)], pa=PA)), "pre[0]: col = -1"),
        (call(flow, 3, _args(pre=[(0, 0, L.PGM_PRE_COPY, 0.0, 0.0, 0.0, 1.0)], pa=PA)), "pre[0]: col = 0 (+0)"),
        (call(flow, 3, _args(pre=[(0, 1, 2, 0.0, 0.0, 0.0, 1.0)], cf_pa=CFPA)), "pre[0]: unknown kind 2"),
        (call(flow, 3, _args(pre=[(0, 1, L.PGM_PRE_LOGSTD, 2.0, 1.0, 0.0, 0.0)], cf_pa=CFPA)), "pre[0]: sd = 0"),
        (call(flow, 3, _args(rows=0)), "rows = 0"),
        (call(flow, 3, _args(table_rows=7)), "table_rows = 7"),
        (call(flow, 3, _args(ncol=0)), "ncol = 0"),
        (call(flow, 3, _args(ncol=2)), "col = 2 (+1) is out of range (ncol = 2)"),
        (call(flow, 0, _args()), "n = 0"),
        (call(None, 1, _args()), "null mechanism records"),
        (call(_recs(root(0), root(1), aff(width=[65])), 3, _args()), "width[0] = 65"),
        (call(_recs(root(0), root(1), aff(p=[P, P, P, P, P, 0])), 3, _args()), "null parameter pointer p[5]"),
    ]
    for (rc, msg), words in cases:
        assert rc < 0 and words in msg and "cgen_pgm_counterfactual" in msg, (words, rc, msg)
