"""Without a GPU: the case table of tests/test_gpu_elementwise.py reaches every launch arm of every element-wise entry point in
both dtypes, including the edges the arms get wrong (channel-slice views, accumulation, grid-stride wrap), and the Python mirror
of the host-side arm choice still reads like the C it mirrors."""
import os
import re
from collections import defaultdict

import pytest

import elementwise_cases as E
from conftest import ROOT


def _covered():
    cov = defaultdict(list)
    for c in E.CASES:
        for a, _ in E.launch_arms(c):
            cov[(c.op, c.dt, a)].append(c)
    return cov


def test_case_ids_are_unique():
    ids = [c.id() for c in E.CASES]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("op", E.TV_OPS + E.PLAIN_OPS)
@pytest.mark.parametrize("dt", E.DTYPES)
def test_every_arm_is_reached(op, dt):
    cov = _covered()
    for a in E.ALL_ARMS[op]:
        assert cov[(op, dt, a)], (op, dt, a)


@pytest.mark.parametrize("op", E.TV_OPS)
@pytest.mark.parametrize("dt", E.DTYPES)
def test_vector_ops_see_both_scalar_routes_and_vector_slices(op, dt):
    cases = [c for c in E.CASES if c.op == op and c.dt == dt and not c.flat_axpy]
    scalar = [c for c in cases if E.arm(c) == "scalar"]
    assert any(c.c % 4 for c in scalar), "scalar by c % 4"
    assert {c.off for c in scalar if c.c % 4 == 0} >= {1, 2, 3}, "scalar by a channel offset of 1, 2 and 3"
    # a 4-channel store into a slice of a wider tensor: the neighbouring channels must survive it
    assert any(E.arm(c) == "vec" and c.off and c.cext for c in cases)
    if op in E.ACC_OPS:
        for a in ("vec", "scalar"):
            assert {c.acc for c in cases if E.arm(c) == a} == {0, 1}, a


@pytest.mark.parametrize("op", E.TV_OPS + E.PLAIN_OPS)
def test_every_arm_wraps_the_grid_somewhere(op):
    wrapped = {a for c in E.CASES if c.op == op and E.wraps(c) for a, items in E.launch_arms(c)
               if items > (E.BATCH_REDUCE_CAP if op == "batch_reduce" else E.GRID_CAP)}
    assert wrapped >= E.ALL_ARMS[op], (op, wrapped)


def test_axpby_edges():
    cases = [c for c in E.CASES if c.op == "axpby"]
    for dt in E.DTYPES:
        # c_from inside a 4-channel group of the vector arm, with a beta that changes the result
        assert any(E.arm(c) == "vec" and c.dt == dt and c.p[2] < c.c and c.p[2] % 4 and c.p[1] != 1.0 and not c.p[3] for c in cases)
        assert any(E.arm(c) == "scalar" and c.dt == dt and c.p[2] < c.c and c.p[1] != 1.0 for c in cases)
        for a in ("vec", "scalar", "flat"):  # fills (in = NULL) in every arm, into a zero and a non-zero destination
            assert {c.acc for c in cases if c.dt == dt and c.p[3] and E.arm(c) == a} == {0, 1}, (dt, a)
    tails = [E.launch_arms(c) for c in cases if c.flat_axpy]
    assert any([a for a, _ in t] == ["flat", "scalar"] for t in tails)  # count % 1024 % 4 != 0: a scalar tail
    assert any([a for a, _ in t] == ["flat", "flat"] for t in tails)
    assert any([a for a, _ in t] == ["scalar"] for t in tails)  # fewer than 1024


def test_plain_op_edges():
    for dt in E.DTYPES:
        br = [c for c in E.CASES if c.op == "batch_reduce" and c.dt == dt]
        assert {c.acc for c in br} == {0, 1} and any(c.p[0] != 1.0 for c in br) and any(c.n % 4 for c in br)
        for op in ("im2col_strided", "col2im_strided"):
            cs = [c for c in E.CASES if c.op == op and c.dt == dt]
            assert {c.p[0] for c in cs} >= {3, 5} and all(c.p[1] == 2 for c in cs)
            assert any(c.h % 2 and c.w % 2 for c in cs)
        assert {c.acc for c in E.CASES if c.op == "col2im_strided" and c.dt == dt} == {0, 1}
        for u in E.UNARY:
            assert {c.acc for c in E.CASES if c.op == "unary_bwd" and c.dt == dt and c.p[0] == u} == {0, 1}
            assert any(c.op == "unary_fwd" and c.dt == dt and c.p[0] == u for c in E.CASES)
        srcs = {c.p[0] for c in E.CASES if c.op == "nchw_to_nhwc" and c.dt == dt}
        assert srcs == {"f32", "u8"}


def test_mirror_matches_the_host_code():
    """The predicates above are copied from elementwise.hip; a change there must be carried over here."""
    src = open(os.path.join(ROOT, "causal-gen_amd", "csrc", "elementwise.hip")).read()
    vec = re.search(r"static inline bool vec4_ok\(.*?\n}\n", src, re.S).group(0)
    assert "if (c % 4) return false;" in vec and "const int q = 4 * esz;" in vec
    assert "((uintptr_t)v->p % q) || ((v->sn * esz) % q) || ((v->sh * esz) % q) || ((v->sw * esz) % q)" in vec
    assert "if (!v || !v->p) continue;" in vec
    assert "if (b > 256 * 16) b = 256 * 16;" in src  # GRID_CAP
    assert "return v.sw == c && v.sh == (int64_t)w * c && v.sn == (int64_t)h * w * c && ((uintptr_t)v.p % 16) == 0;" in src
    assert "if (c % (16 / esz) == 0 && c_from >= c && flat(out) && (!in.p || (flat(in) && in.c == c))) {" in src
    eng = open(os.path.join(ROOT, "causal-gen_amd", "engine.py")).read()
    assert "cols = 1024" in eng  # Engine.flat_axpy, mirrored by flat_axpy_calls


def test_mirror_decisions():
    # f32: 16-byte groups; 16-bit: 8-byte groups, so a slice at offset 4 keeps the vector arm in both
    assert E.vec4_ok(4, 8, [(16, 16 * 35, 16 * 5, 16)]) and not E.vec4_ok(4, 8, [(8, 16 * 35, 16 * 5, 16)])
    assert E.vec4_ok(2, 8, [(8, 16 * 35, 16 * 5, 16)]) and not E.vec4_ok(2, 8, [(4, 16 * 35, 16 * 5, 16)])
    assert not E.vec4_ok(4, 8, [(0, 9 * 35, 9 * 5, 9)])  # odd pixel stride
    assert not E.vec4_ok(4, 6, [(0, 0, 0, 8)])
    assert E.axpby_flat(4, 1, 1, 3, 1024, E.NO_SPLIT, [(0, 3072, 3072, 1024)] * 2)
    assert not E.axpby_flat(4, 1, 1, 3, 1024, 1000, [(0, 3072, 3072, 1024)] * 2)
    assert not E.axpby_flat(2, 3, 7, 5, 12, E.NO_SPLIT, [(0, 420, 60, 12)] * 2)  # 12 halves: not whole 16-byte vectors
