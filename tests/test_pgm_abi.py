"""The parent-SCM entry points without a GPU: exported, declared and bound at ABI 411, eight mechanism records fit the
kernel-argument segment, the workspace query follows the slot counts, every entry rejects bad arguments before anything is launched
with a message naming the field, and PgmTrainStep's record builder refuses a PGM the kernel does not serve."""
import ctypes as C
import os
import re

import pytest

import pgm_cases as PC
from conftest import ROOT

ENTRIES = ("cgen_pgm_workspace", "cgen_pgm_nll_fwd", "cgen_pgm_nll_fwd_bwd")
OBS, TERMS, LOSS, COEF, WS, P = 8192, 12288, 16384, 20480, 24576, 4096  # fake device addresses: validation must reject before any use


def _mech(kind, **kw):
    from causal_gen_amd import _lib

    r = _lib.PgmMech()
    r.kind, r.col, r.ncls, r.nctx, r.nhidden, r.act, r.bins, r.bound = kind, 0, 2, 1, 1, 0, 4, 3.0
    r.width[0] = 8
    for i in range(8):
        r.p[i], r.g[i] = P, P
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


def test_symbols_exported_declared_and_bound_at_abi_411():
    from causal_gen_amd import _lib

    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "cgen_hip.h")).read()
    assert "#define CGEN_ABI_VERSION 411" in hdr and lib.version() == 411 == _lib.ABI_VERSION
    for name in ENTRIES:
        assert re.search(r"\bint %s\(const cgen_pgm_mech\* mechs," % name, hdr), name
        assert hasattr(lib.cdll, name) and name in _lib.PROTOTYPES, name
    assert "typedef struct cgen_pgm_mech {" in hdr


def test_mechanism_records_fit_the_kernel_argument_segment():
    """(the record's layout and the constants against the header: tests/test_abi_mirror.py)"""
    from causal_gen_amd import _lib

    assert C.sizeof(_lib.PgmMech) * _lib.PGM_MAX_MECH < 3500  # eight records travel by value in a 4 KiB kernel-argument segment


def test_workspace_follows_the_slot_counts():
    from causal_gen_amd import _lib

    lib = _lib.load()
    L = _lib
    # FlowPGM's shape: two Bernoulli roots, a 4-bin spline, two MLPs 2 -> 32 -> 32 -> 2
    mlp = lambda: _mech(L.PGM_AFFINE, nctx=2, nhidden=2, width=[32, 32])
    flow = _recs(_mech(L.PGM_BERNOULLI), _mech(L.PGM_BERNOULLI), _mech(L.PGM_SPLINE, bins=4), mlp(), mlp())
    flow_slots = 1 + 1 + (4 * 4 + 3) + 2 * ((32 * 2 + 32) + (32 * 32 + 32) + (2 * 32 + 2))
    # ChestPGM's: a Bernoulli root, an 8-bin spline, a 3-class root, a Gumbel-max MLP 1 -> 8 -> 16 -> 2 with Sigmoid
    chest = _recs(_mech(L.PGM_BERNOULLI), _mech(L.PGM_SPLINE, bins=8), _mech(L.PGM_CATEGORICAL, ncls=3),
                  _mech(L.PGM_GUMBEL_MAX, ncls=2, nctx=1, nhidden=2, width=[8, 16], act=L.PGM_SIGMOID))
    chest_slots = 1 + (4 * 8 + 3) + 3 + ((8 * 1 + 8) + (16 * 8 + 16) + (2 * 16 + 2))
    for recs, slots in ((flow, flow_slots), (chest, chest_slots)):
        for rows, blocks in ((1, 1), (64, 1), (65, 2), (129, 3), (1024, 16)):
            got = L.i64(-1)
            lib.pgm_workspace(recs, len(recs), rows, C.byref(got))
            assert got.value == 4 * slots * blocks, (slots, rows, got.value)
    with pytest.raises(L.CgenError, match="null output"):
        lib.pgm_workspace(flow, 5, 8, None)
    with pytest.raises(L.CgenError, match="rows = 0"):
        lib.pgm_workspace(flow, 5, 0, C.byref(L.i64(0)))


def test_entry_points_reject_bad_arguments_before_launch():
    from causal_gen_amd import _lib

    lib, L = _lib.load(), _lib

    def all3(recs, n, ncol=4, rows=8, obs=OBS, terms=TERMS, loss=LOSS, coef=COEF, ws=WS, ws_bytes=1 << 40, table_rows=8, query=True, fwd=True):
        """fwd=False: a record that is VALID for cgen_pgm_nll_fwd -- that call would launch on the stand-in addresses where a GPU is present."""
        out = []
        if query:
            rc = lib._raw_cgen_pgm_workspace(recs, n, rows, C.byref(L.i64(0)))
            out.append((rc, lib.last_error().decode()))
        if fwd:
            rc = lib._raw_cgen_pgm_nll_fwd(recs, n, obs, ncol, table_rows, None, rows, terms, loss, None)
            out.append((rc, lib.last_error().decode()))
        rc = lib._raw_cgen_pgm_nll_fwd_bwd(recs, n, obs, ncol, table_rows, None, rows, terms, loss, coef, ws, ws_bytes, None)
        out.append((rc, lib.last_error().decode()))
        return out

    good = _mech(L.PGM_AFFINE, nctx=2, ctx_col=[1, 2], nhidden=2, width=[32, 32])
    cases = [
        (all3(_recs(_mech(L.PGM_AFFINE, width=[65])), 1), "width[0] = 65"),
        (all3(_recs(_mech(L.PGM_GUMBEL_MAX, nhidden=2, width=[8, 0])), 1), "width[1] = 0"),
        (all3(_recs(_mech(L.PGM_AFFINE, nhidden=4)), 1), "nhidden = 4"),
        (all3(_recs(_mech(L.PGM_AFFINE, nhidden=0)), 1), "nhidden = 0"),
        (all3(_recs(_mech(L.PGM_SPLINE, bins=9)), 1), "bins = 9"),
        (all3(_recs(_mech(L.PGM_SPLINE, bound=0.0)), 1), "bound = 0"),
        (all3(_recs(_mech(7)), 1), "unknown kind 7"),
        (all3(_recs(_mech(-1)), 1), "unknown kind -1"),
        (all3(_recs(_mech(L.PGM_AFFINE, act=3)), 1), "unknown act 3"),
        (all3(_recs(_mech(L.PGM_AFFINE, nctx=3)), 1), "nctx = 3"),
        (all3(_recs(_mech(L.PGM_CATEGORICAL, ncls=17)), 1), "ncls = 17"),
        (all3(_recs(_mech(L.PGM_SPLINE, normalize=2)), 1), "normalize = 2"),
        (all3(_recs(good), 0), "n = 0"),
        (all3(_recs(good), 9), "n = 9"),
        (all3(None, 1), "null mechanism records"),
        # the columns are the batch entries' business: the workspace query does not see the table
        (all3(_recs(_mech(L.PGM_BERNOULLI, col=4)), 1, query=False), "col = 4"),
        (all3(_recs(_mech(L.PGM_BERNOULLI, col=-1)), 1, query=False), "col = -1"),
        (all3(_recs(_mech(L.PGM_CATEGORICAL, ncls=3, col=2)), 1, query=False), "col = 2 (+3)"),
        (all3(_recs(_mech(L.PGM_AFFINE, nctx=2, ctx_col=[1, 4])), 1, query=False), "ctx_col[1] = 4"),
        (all3(_recs(good), 1, obs=None, query=False), "null obs"),
        (all3(_recs(good), 1, terms=None, query=False), "null terms"),
        (all3(_recs(good), 1, loss=None, query=False), "null loss_sum"),
        (all3(_recs(good), 1, rows=0), "rows = 0"),
        (all3(_recs(good), 1, table_rows=7, query=False), "table_rows = 7"),
        (all3(_recs(_mech(L.PGM_SPLINE, p=[P, P, P, 0])), 1, query=False), "null parameter pointer p[3]"),
    ]
    for res, words in cases:
        for rc, msg in res:
            assert rc < 0 and words in msg, (words, msg)
    one = _recs(good)
    for kw, words in ((dict(coef=None), "null coef_dev"), (dict(ws=None), "null workspace"), (dict(ws_bytes=4 * 1218 - 1), "workspace too small")):
        rc, msg = all3(one, 1, fwd=False, **kw)[-1]
        assert rc < 0 and words in msg, (words, msg)
    nog = _mech(L.PGM_AFFINE, nctx=2, ctx_col=[1, 2], nhidden=2, width=[32, 32], g=[P, P, P, P, 0, P])
    rc, msg = all3(_recs(nog), 1, fwd=False)[-1]
    assert rc < 0 and "null gradient pointer g[4]" in msg, msg


def test_record_builder_mirrors_the_pgm_and_refuses_what_the_kernel_does_not_serve():
    """(no GPU: build_records only takes addresses)"""
    import torch

    from causal_gen_amd import _lib
    from causal_gen_amd import pgm as P_
    from causal_gen_amd import pgm_train as PT

    L = _lib
    m = PC.make_pgm("flow")
    cols, ncol = PT.default_columns(m)
    assert cols == {"sex": 0, "mri_seq": 1, "age": 2, "brain_volume": 3, "ventricle_volume": 4} and ncol == 5
    recs = PT.build_records(m, cols, ncol)
    assert [r.kind for r in recs] == [L.PGM_BERNOULLI, L.PGM_BERNOULLI, L.PGM_SPLINE, L.PGM_AFFINE, L.PGM_AFFINE]
    v = recs[4]
    assert (v.col, v.nctx, list(v.ctx_col), v.nhidden, list(v.width)[:2], v.act, v.normalize) == (4, 2, [3, 2], 2, [32, 32], L.PGM_LEAKY_RELU, 0)
    assert v.p[0] == m.vvol_flow.context_nn.layers[0].weight.data_ptr() and v.p[5] == m.vvol_flow.context_nn.layers[2].bias.data_ptr()
    assert (recs[2].bins, recs[2].bound, recs[2].p[3]) == (4, 3.0, m.age_module[0].unnormalized_lambdas.data_ptr())
    m = PC.make_pgm("morpho")
    cols, ncol = PT.default_columns(m)
    assert cols == {"thickness": 0, "intensity": 1, "digit": 2} and ncol == 12
    recs = PT.build_records(m, cols, ncol)
    assert [(r.kind, r.normalize, r.col) for r in recs] == [(L.PGM_CATEGORICAL, 0, 2), (L.PGM_SPLINE, 1, 0), (L.PGM_AFFINE, 1, 1)]
    assert recs[0].ncls == 10 and recs[2].act == L.PGM_GELU and list(recs[2].ctx_col)[:1] == [0]
    m = PC.make_pgm("chest")
    recs = PT.build_records(m, *PT.default_columns(m))
    assert [(r.kind, r.col) for r in recs] == [(L.PGM_BERNOULLI, 3), (L.PGM_SPLINE, 5), (L.PGM_CATEGORICAL, 0), (L.PGM_GUMBEL_MAX, 4)]
    assert (recs[1].bins, recs[3].ncls, recs[3].act, list(recs[3].width)[:2]) == (8, 2, L.PGM_SIGMOID, [8, 16])
    # what the kernel does not serve is an error that says so, never a fall-back
    for widths, words in (([128], "widths up to 64"), ([8, 8, 8, 8], "4 hidden layers")):
        with pytest.raises(ValueError, match=words):
            m = PC.make_pgm("flow", widths=widths)
            PT.build_records(m, *PT.default_columns(m))
    m = PC.make_pgm("chest")
    m.age_flow_components[0] = P_.LinearSpline(1, count_bins=16)
    with pytest.raises(ValueError, match="16 bins"):
        PT.build_records(m, *PT.default_columns(m))
    m = PC.make_pgm("morpho")
    m.context_nn.context_nn.f = torch.nn.Tanh()
    with pytest.raises(ValueError, match="LeakyReLU"):
        PT.build_records(m, *PT.default_columns(m))
    m = PC.make_pgm("flow")
    with pytest.raises(ValueError, match="no column was named for variable 'age'"):
        PT.build_records(m, {"sex": 0, "mri_seq": 1, "brain_volume": 2, "ventricle_volume": 3}, 4)
    with pytest.raises(ValueError, match="do not fit a table of 4 columns"):
        PT.build_records(m, PT.default_columns(m)[0], 4)
    with pytest.raises(ValueError, match="lr_warmup_steps"):
        PT.PgmTrainStep(m, lr_warmup_steps=0)
