"""``cgen_philox_uniform`` against the numpy twin of the in-kernel generator (tests/test_gpu_ops.py), and
``PgmCounterfactual.run(rng=)``: the Gumbel-max uniforms of ChestPGM's ``finding | age`` drawn on the device from the engine's
``{seed, offset}`` state instead of torch's generator.

Counts: 1, 3, 4, 5 (a partial and a full group of four), 1023 / 1025 (a partial group at a workgroup's edge, more than one
workgroup) and 4096 x 1024 + 5: the grid is capped at 4096 workgroups of 256 threads x 4 values, so the grid-stride loop takes a
second trip.  Everything is bit-equality: the kernel computes u01 in f32 exactly as the twin does."""
import numpy as np
import pytest
import torch

import chest_cf_fixture as FX
import pgm_cases as PC
from test_gpu_ops import _philox_words, _u01

pytestmark = pytest.mark.gpu

STATES = [(1234567, 3), (0x123456789ABC, (5 << 32) + 7)]  # the second offset has a non-zero high word
STREAMS = [989, 3]
GUARD = 8


def _twin(seed, offset, stream, count):
    groups = np.arange((count + 3) // 4, dtype=np.uint64)
    return _u01(_philox_words(seed, offset, stream, groups)).reshape(-1)[:count]


def _fill(lib, count, rng, stream):
    out = torch.full((count + GUARD,), -1.0, device="cuda")
    lib.philox_uniform(out.data_ptr(), count, rng.data_ptr(), stream, torch.cuda.current_stream().cuda_stream)
    return out


@pytest.mark.parametrize("count", [1, 3, 4, 5, 1023, 1025, 4096 * 1024 + 5])
def test_philox_uniform_equals_the_numpy_twin(count):
    from causal_gen_amd import _lib

    lib = _lib.require_gpu()
    combos = [(s, st) for s in STATES for st in STREAMS] if count < 10 ** 6 else [(STATES[1], STREAMS[0])]
    for (seed, offset), stream in combos:
        rng = torch.tensor([seed, offset], dtype=torch.int64, device="cuda")
        before = rng.clone()
        got = _fill(lib, count, rng, stream)
        again = _fill(lib, count, rng, stream)
        torch.cuda.synchronize()
        assert torch.equal(rng, before)  # the state is read, not advanced
        assert torch.equal(got, again)
        assert bool((got[count:] == -1.0).all())  # nothing past `count`
        g = got[:count].cpu().numpy()
        want = _twin(seed, offset, stream, count)
        assert g.dtype == want.dtype == np.float32 and np.array_equal(g.view(np.uint32), want.view(np.uint32)), (count, seed, offset, stream)
        assert float(g.min()) > 0.0 and float(g.max()) < 1.0 and bool(np.isfinite(np.log(-np.log(g.astype(np.float64)))).all())
    if count >= 10 ** 6:
        assert count > 4096 * 256 * 4  # (the second trip of the grid-stride loop)
        other = _fill(lib, 16, torch.tensor(list(STATES[0]), dtype=torch.int64, device="cuda"), 989)[:16]
        assert not torch.equal(other, got[:16])  # another state: other values


# ------------------------------------------------------------------------------------------------ PgmCounterfactual.run(rng=)
def _runner():
    from types import SimpleNamespace

    from causal_gen_amd.pgm_cf import PgmCounterfactual

    scm = PC.make_pgm("chest", seed=0)
    args = SimpleNamespace(parents_x=["age", "race", "sex", "finding"], dataset="mimic")
    cfm = PgmCounterfactual(scm, args)
    _, table = FX.dataset(device="cpu")
    return cfm, table.cuda().contiguous()


def _outs(cfm, res, B):
    torch.cuda.synchronize()
    return [t.clone() for t in res] + [cfm.noise(B).clone()]


def _equal(a, b):
    return all(torch.equal(FX.bits(x), FX.bits(y)) for x, y in zip(a, b))


def test_run_with_rng_equals_run_with_the_twins_uniforms_and_replays_at_the_new_offset():
    from causal_gen_amd import _lib, step_tail

    lib = _lib.require_gpu()
    cfm, table = _runner()
    B = table.shape[0]
    perm = torch.tensor([3, 0, 7, 1, 6, 2, 5, 4], device="cuda")
    seed, offset = STATES[1]
    rng = torch.tensor([seed, offset], dtype=torch.int64, device="cuda")
    assert cfm.gumbel == [cfm.vars.index("finding")] and tuple(cfm._entry(B)["uniforms"][cfm.gumbel[0]].shape) == (B, 2)

    def twin(off):
        return torch.from_numpy(_twin(seed, off, _lib.STREAM_GUMBEL, 2 * B).reshape(B, 2).copy()).cuda()

    torch.manual_seed(0)
    state = torch.cuda.get_rng_state()
    got = _outs(cfm, cfm.run(table, None, table, perm, do_vars=["age"], rng=rng), B)
    assert torch.equal(torch.cuda.get_rng_state(), state)  # torch's generator drew nothing
    assert torch.equal(FX.bits(cfm._entry(B)["uniforms"][cfm.gumbel[0]]), FX.bits(twin(offset)))
    want = _outs(cfm, cfm.run(table, None, table, perm, do_vars=["age"], uniforms=twin(offset)), B)
    assert _equal(got, want)
    cf = got[0]
    assert torch.equal(FX.bits(cf[:, 5]), FX.bits(table[perm, 5]))  # age: the do rows' bits
    assert bool(((cf[:, 4] == 0) | (cf[:, 4] == 1)).all())

    # captured: a replay after cgen_rng_advance draws at the new offset
    graph, res = step_tail.capture(lambda: cfm.run(table, None, table, perm, do_vars=["age"], rng=rng))
    lib.rng_advance(rng.data_ptr(), 3, torch.cuda.current_stream().cuda_stream)
    graph.replay()
    replayed = _outs(cfm, res, B)
    assert int(rng[1]) == offset + 3
    eager = _outs(cfm, cfm.run(table, None, table, perm, do_vars=["age"], rng=rng), B)
    want3 = _outs(cfm, cfm.run(table, None, table, perm, do_vars=["age"], uniforms=twin(offset + 3)), B)
    assert _equal(replayed, eager) and _equal(replayed, want3)
    assert not torch.equal(twin(offset), twin(offset + 3))


def test_uniforms_and_rng_together_raise_and_do_sex_leaves_finding_as_observed():
    cfm, table = _runner()
    B = table.shape[0]
    perm = torch.arange(B - 1, -1, -1, device="cuda")
    rng = torch.tensor(list(STATES[0]), dtype=torch.int64, device="cuda")
    u = torch.rand(B, 2, device="cuda")
    with pytest.raises(ValueError, match="not both"):
        cfm.run(table, None, table, perm, do_vars=["age"], uniforms=u, rng=rng)
    with pytest.raises(ValueError, match="not both"):
        cfm.run(table, None, table, perm, do_vars=["age"], uniforms={"finding": u}, rng=rng)
    with pytest.raises(ValueError, match="rng must be"):
        cfm.run(table, None, table, perm, do_vars=["age"], rng=rng.cpu())
    for state in STATES:  # whatever is drawn, finding is not downstream of sex: the observation's bits
        rng.copy_(torch.tensor(list(state), dtype=torch.int64))
        cf = cfm.run(table, None, table, perm, do_vars=["sex"], rng=rng)[0]
        torch.cuda.synchronize()
        assert torch.equal(FX.bits(cf[:, 4]), FX.bits(table[:, 4])) and torch.equal(FX.bits(cf[:, 3]), FX.bits(table[perm, 3]))
        assert torch.equal(FX.bits(cf[:, 5]), FX.bits(table[:, 5])) and torch.equal(FX.bits(cf[:, :3]), FX.bits(table[:, :3]))
