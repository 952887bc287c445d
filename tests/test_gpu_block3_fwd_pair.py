"""cgen_block3_pair with two FORWARD records (pre_act = 1): a decoder layer's posterior and prior Blocks in one launch, through the C
ABI.  The pair launch against the two single launches of the same records, every tensor between guard bands in one patterned
buffer: equal bytes for both outputs and both bottleneck tensors, inputs and guard bands untouched; every combination the entry
points decline answers 0 (as without a GPU: tests/test_pairing_fwd.py asks the same records), raises on launch and writes nothing."""
import ctypes as C
import math

import pytest
import torch

import fwd_pair_cases as fc

pytestmark = pytest.mark.gpu

GUARD = 4096  # bytes between two tensors, and at both ends


def _problem(shape, seed=0):
    """Engine-made weight images of the two Blocks, and one int16 buffer holding every tensor of both records."""
    from causal_gen_amd.engine import ConvSite, Engine

    g = torch.Generator().manual_seed(17 + seed)
    convs, sites = [], []
    for k, rec in enumerate((shape.a, shape.b)):
        ci = sum(rec.seg_c)
        c1, c2 = torch.nn.Conv2d(ci, rec.b, 3, padding=1), torch.nn.Conv2d(rec.b, rec.co, 3, padding=1)
        with torch.no_grad():
            c1.weight.copy_(torch.randn(c1.weight.shape, generator=g) / math.sqrt(ci * 9 / 2))
            c2.weight.copy_(torch.randn(c2.weight.shape, generator=g) / math.sqrt(rec.b * 9 / 2))
            c1.bias.copy_(torch.randn(rec.b, generator=g) * 0.2)
            c2.bias.copy_(torch.randn(rec.co, generator=g) * 0.2)
        convs += [c1, c2]
    holder = torch.nn.ModuleList(convs).cuda()
    for k, rec in enumerate((shape.a, shape.b)):
        s1 = ConvSite("c%d1" % k, holder[2 * k], rec.seg_c, [True] * len(rec.seg_c), 2 * k)
        s2 = ConvSite("c%d2" % k, holder[2 * k + 1], [rec.b], [True], 2 * k + 1)
        s1.blk3, s2.blk3 = ("a", s2), ("b", s1)
        sites += [s1, s2]
    eng = Engine("cuda", "f16")
    eng.blk3_on = 2
    eng.bind(holder, sites)
    eng.begin()
    eng.prepare_weights(force=True)
    # ---- the buffer: [guard] tensor [guard] tensor ... [guard]; inputs random, everything else a position-dependent pattern
    n, h, w = shape.n, shape.h, shape.w
    regions, off = {}, GUARD

    def place(name, c):
        nonlocal off
        nbytes = fc.tensor_bytes(n, h, w, c)
        regions[name] = (off, nbytes)
        off += (nbytes + 255) // 256 * 256 + GUARD

    for k, rec in enumerate((shape.a, shape.b)):
        for j, c in enumerate(rec.seg_c):
            place("seg%d%d" % (k, j), c)
        place("mid%d" % k, rec.b)
        place("out%d" % k, rec.co)
    buf = ((torch.arange(off // 2, dtype=torch.int32) % 251) + 0x3000).to(torch.int16).cuda()  # (binary16 in [0.125, 0.25): finite)
    inputs = []
    for k, rec in enumerate((shape.a, shape.b)):
        for j, c in enumerate(rec.seg_c):
            o, nb = regions["seg%d%d" % (k, j)]
            if c % 8:  # the parents: [n][8], channels c .. 7 zero
                v = torch.zeros(n, 8)
                v[:, :c] = torch.randn(n, c, generator=g)
            else:
                v = torch.randn(nb // 2, generator=g)
            buf[o // 2:(o + nb) // 2] = v.half().view(torch.int16).flatten().cuda()
            inputs.append((o, nb))
    base = buf.data_ptr()
    ptrs = []
    for k, rec in enumerate((shape.a, shape.b)):
        s1, s2 = sites[2 * k], sites[2 * k + 1]
        ptrs.append({"seg": [base + regions["seg%d%d" % (k, j)][0] for j in range(len(rec.seg_c))],
                     "mid": base + regions["mid%d" % k][0], "out": base + regions["out%d" % k][0],
                     "w_a": s1.frag["a_fwd"], "bias_a": s1.conv.bias.data_ptr(), "w_b": s2.frag["b_fwd"], "bias_b": s2.conv.bias.data_ptr()})
    return eng, holder, buf, regions, ptrs


@pytest.mark.parametrize("shape", fc.SHAPES, ids=[s.name for s in fc.SHAPES])
def test_forward_pair_launch_has_the_bytes_of_the_two_single_launches(shape):
    eng, holder, buf, regions, (pa, pb) = _problem(shape)
    lib = eng.lib
    a, b = fc.args(shape.n, shape.h, shape.w, shape.a, pa), fc.args(shape.n, shape.h, shape.w, shape.b, pb)
    assert lib.block3_supported(C.byref(a)) == 1 and lib.block3_supported(C.byref(b)) == 1
    ok, plan = fc.plan(lib, a, b)
    assert ok == 1 and plan == shape.plan, plan  # (the instances this case is here for; na = plan[4] workgroups take record A)
    assert lib.block3_pair_supported(C.byref(a), C.byref(b)) == 1
    init = buf.clone()
    lib.block3(C.byref(a), eng.stream)
    lib.block3(C.byref(b), eng.stream)
    torch.cuda.synchronize()
    ref = buf.clone()
    buf.copy_(init)
    lib.block3_pair(C.byref(a), C.byref(b), eng.stream)
    torch.cuda.synchronize()
    written = torch.zeros_like(buf, dtype=torch.bool)
    for name in ("mid0", "out0", "mid1", "out1"):
        o, nb = regions[name]
        assert torch.equal(buf[o // 2:(o + nb) // 2], ref[o // 2:(o + nb) // 2]), name  # equal bytes
        changed = (ref[o // 2:(o + nb) // 2] != init[o // 2:(o + nb) // 2]).float().mean().item()
        assert changed > 0.4 if name.startswith("out") else changed > 0.1, (name, changed)  # (the launches did write them; a ReLU'd bottleneck is half zeros ... of a pattern that has none)
        written[o // 2:(o + nb) // 2] = True
    # inputs and guard bands: the bytes they had, after the single launches and after the pair
    assert torch.equal(buf[~written], init[~written]) and torch.equal(ref[~written], init[~written])
    assert torch.isfinite(buf[written].view(torch.float16).float()).all()


def test_declined_pairs_answer_zero_launch_nothing_and_write_nothing():
    shape = fc.SHAPES[0]
    eng, holder, buf, regions, (pa, pb) = _problem(shape)
    lib = eng.lib
    from causal_gen_amd._lib import CgenError

    init = buf.clone()
    cases = fc.declined(shape.n, shape.h, shape.w, shape.a, shape.b, pa, pb) + [("row-streaming",) + fc.row_streaming()]
    cpu = fc.declined(shape.n, shape.h, shape.w, shape.a, shape.b) + [("row-streaming",) + fc.row_streaming()]
    for (name, a, b), (_, ca, cb) in zip(cases, cpu):
        assert lib.block3_pair_supported(C.byref(a), C.byref(b)) == 0, name
        assert lib.block3_pair_supported(C.byref(ca), C.byref(cb)) == 0, name  # (the same records on stand-in addresses: host code)
        n0 = eng.launches
        with pytest.raises(CgenError):
            lib.block3_pair(C.byref(a), C.byref(b), eng.stream)
        assert eng.launches == n0
    torch.cuda.synchronize()
    assert torch.equal(buf, init)
    # ... and the served pair still is
    a, b = fc.args(shape.n, shape.h, shape.w, shape.a, pa), fc.args(shape.n, shape.h, shape.w, shape.b, pb)
    assert lib.block3_pair_supported(C.byref(a), C.byref(b)) == 1
