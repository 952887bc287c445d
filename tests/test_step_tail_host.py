"""step_tail.StepTail without a GPU: CPU tensors and a stub library that records every call.  The launch sequence and every field of
every ``AdamwArgs`` are compared with lists written out here from what the three training steps issued before they shared the tail
(TrainStep: one adamw_ema per used range; PredictorTrainStep: the whole buffer, then the running statistics with lr = wd = 0 on a
zero gradient; PgmTrainStep: the whole buffer, 64 partial sums, no norm threshold).  Also ``check_warmup`` and ``flatten``."""
import numpy as np
import pytest
import torch

ST = 77  # the stream handle: passed through to every launch
FIELDS = ("p", "g", "m", "v", "ema", "count", "lr", "beta1", "beta2", "eps", "wd", "ema_beta", "warmup_steps", "ema_update_after", "state_dev")


def f32(v):
    return float(np.float32(v))


class StubLib:
    def __init__(self):
        self.calls = []

    def sumsq_partial(self, *a):
        self.calls.append(("sumsq_partial", a))

    def clip_decide(self, *a):
        self.calls.append(("clip_decide", a))

    def adamw_ema(self, ref, st):
        self.calls.append(("adamw_ema", ({k: getattr(ref._obj, k) for k in FIELDS}, st)))  # (the fields copied out)

    def step_commit(self, *a):
        self.calls.append(("step_commit", a))


def _setup(n, nblk, **hp):
    from causal_gen_amd.step_tail import HyperParams, StepTail

    lib = StubLib()
    tail = StepTail(lib, n, "cpu", nblk)
    assert tail.m.shape == tail.v.shape == (n,) and tail.state.shape == (8,) and tail.partial.shape == (nblk,)
    assert tail.m.dtype == tail.v.dtype == tail.state.dtype == tail.partial.dtype == torch.float32
    assert not tail.m.any() and not tail.v.any() and not tail.state.any()
    kw = dict(lr=1e-3, betas=(0.9, 0.95), eps=1e-8, wd=0.01, grad_clip=350.0, grad_skip=500.0, lr_warmup_steps=100, ema_rate=0.999,
              ema_update_after=100)
    kw.update(hp)
    b = {k: torch.zeros(n) for k in ("p", "g", "ema")}
    return lib, tail, HyperParams(**kw), b


def _args(p, g, m, v, ema, count, state, lr=1e-3, wd=0.01, beta2=0.95, eps=1e-8, warmup=100, after=100):
    return dict(p=p, g=g, m=m, v=v, ema=ema, count=count, lr=f32(lr), beta1=f32(0.9), beta2=f32(beta2), eps=f32(eps), wd=f32(wd),
                ema_beta=f32(0.999), warmup_steps=warmup, ema_update_after=after, state_dev=state)


@pytest.mark.parametrize("with_out3", (True, False))
@pytest.mark.parametrize("with_ema", (True, False))
def test_two_ranges_with_a_gap(with_ema, with_out3):
    """TrainStep's use: 12 elements, used ranges [0, 5) and [9, 12); the norm is of all 12."""
    lib, tail, hp, b = _setup(12, 1024)
    out3 = torch.zeros(3) if with_out3 else None
    tail.run(hp, b["p"], b["g"], b["ema"] if with_ema else None, out3, ST, ranges=[(0, 5), (9, 12)])
    P, G, E = (b[k].data_ptr() for k in ("p", "g", "ema"))
    M, V, S, PART = tail.m.data_ptr(), tail.v.data_ptr(), tail.state.data_ptr(), tail.partial.data_ptr()
    assert lib.calls == [
        ("sumsq_partial", (G, 12, PART, 1024, ST)),
        ("clip_decide", (PART, 1024, out3.data_ptr() if with_out3 else None, 350.0, 500.0, S, ST)),
        ("adamw_ema", (_args(P, G, M, V, E if with_ema else None, 5, S), ST)),
        ("adamw_ema", (_args(P + 36, G + 36, M + 36, V + 36, E + 36 if with_ema else None, 3, S), ST)),
        ("step_commit", (S, ST)),
    ]


def test_no_ranges_is_no_update_but_a_step():
    """A model none of whose parameters got a gradient: norm, decision and commit, no adamw_ema."""
    lib, tail, hp, b = _setup(12, 1024)
    tail.run(hp, b["p"], b["g"], b["ema"], None, ST, ranges=[])
    assert [c[0] for c in lib.calls] == ["sumsq_partial", "clip_decide", "step_commit"]


def test_whole_buffer_and_an_ema_only_region():
    """PredictorTrainStep's use: every parameter, then the running statistics (7 floats elsewhere) averaged into their EMA copy."""
    lib, tail, hp, b = _setup(12, 1024, lr=1e-4, wd=0.1, betas=(0.9, 0.999), grad_clip=200.0, grad_skip=float("inf"), lr_warmup_steps=1)
    out3, pb, eb = torch.zeros(3), torch.ones(7), torch.ones(7)
    tail.run(hp, b["p"], b["g"], b["ema"], out3, ST, ema_only=[(pb.data_ptr(), eb.data_ptr(), 7)])
    P, G, E = (b[k].data_ptr() for k in ("p", "g", "ema"))
    M, V, S, PART = tail.m.data_ptr(), tail.v.data_ptr(), tail.state.data_ptr(), tail.partial.data_ptr()
    assert [c[0] for c in lib.calls] == ["sumsq_partial", "clip_decide", "adamw_ema", "adamw_ema", "step_commit"]  # EMA-only BEFORE the commit
    assert lib.calls[0] == ("sumsq_partial", (G, 12, PART, 1024, ST))
    assert lib.calls[1] == ("clip_decide", (PART, 1024, out3.data_ptr(), 200.0, float("inf"), S, ST))
    assert lib.calls[2] == ("adamw_ema", (_args(P, G, M, V, E, 12, S, lr=1e-4, wd=0.1, beta2=0.999, warmup=1), ST))
    q, st = lib.calls[3][1]
    zeros = (q["g"], q["m"], q["v"])
    assert len({*zeros, G, M, V, P, E, pb.data_ptr(), eb.data_ptr()}) == 10  # three buffers of their own
    rows = {row.data_ptr(): row for row in tail._zero}
    assert all(a in rows and rows[a].numel() >= 7 and not rows[a].any() for a in zeros)
    assert (q, st) == (_args(pb.data_ptr(), *zeros, eb.data_ptr(), 7, S, lr=0.0, wd=0.0, beta2=0.999, warmup=1), ST)
    assert lib.calls[4] == ("step_commit", (S, ST))
    # a second step finds the zero buffers where they were (a captured graph holds their addresses)
    tail.run(hp, b["p"], b["g"], b["ema"], out3, ST, ema_only=[(pb.data_ptr(), eb.data_ptr(), 7)])
    assert lib.calls[5:] == lib.calls[:5]
    with pytest.raises(ValueError, match="ema_only"):
        tail.run(hp, b["p"], b["g"], b["ema"], out3, ST, ema_only=[(pb.data_ptr(), eb.data_ptr(), 8)])


def test_whole_buffer_no_norm_threshold_64_partial_sums():
    """PgmTrainStep's use."""
    lib, tail, hp, b = _setup(12, 64, lr=1e-4, wd=0.1, betas=(0.9, 0.999), grad_clip=200.0, grad_skip=float("inf"), lr_warmup_steps=1)
    out3 = torch.zeros(3)
    tail.run(hp, b["p"], b["g"], b["ema"], out3, ST)
    P, G, E = (b[k].data_ptr() for k in ("p", "g", "ema"))
    M, V, S, PART = tail.m.data_ptr(), tail.v.data_ptr(), tail.state.data_ptr(), tail.partial.data_ptr()
    assert lib.calls == [
        ("sumsq_partial", (G, 12, PART, 64, ST)),
        ("clip_decide", (PART, 64, out3.data_ptr(), 200.0, float("inf"), S, ST)),
        ("adamw_ema", (_args(P, G, M, V, E, 12, S, lr=1e-4, wd=0.1, beta2=0.999, warmup=1), ST)),
        ("step_commit", (S, ST)),
    ]


def test_stats_reads_the_named_indices():
    _, tail, _, _ = _setup(4, 64)
    tail.state.copy_(torch.tensor([9.0, 3.0, 0.5, 1.0, 4.0, 17.0, 2.0, 1234.5]))  # (optim.hip's layout)
    assert tail.stats() == dict(grad_norm=3.0, clip_coef=0.5, skipped_last=True, n_skipped=4, opt_steps=17)


def test_flat_optimizer_state_round_trip_and_foreign_names():
    _, a, _, _ = _setup(4, 64)
    _, b, _, _ = _setup(4, 64)
    a.m.copy_(torch.arange(4.0))
    a.v.copy_(torch.arange(4.0) + 10)
    a.state.copy_(torch.arange(8.0))
    sd = a.flat_optimizer_state(["w", "b"])
    assert sorted(sd) == ["exp_avg", "exp_avg_sq", "names", "state"] and sd["names"] == ["w", "b"]
    assert sd["exp_avg"].data_ptr() != a.m.data_ptr()  # a copy, not a view
    b.load_flat_optimizer_state(sd, ["w", "b"])
    assert torch.equal(b.m, a.m) and torch.equal(b.v, a.v) and torch.equal(b.state, a.state)
    with pytest.raises(ValueError, match="belongs to other parameters"):
        b.load_flat_optimizer_state(sd, ["w", "c"])


@pytest.mark.parametrize("n", (0, -5))
def test_check_warmup_raises(n):
    from causal_gen_amd.step_tail import check_warmup

    with pytest.raises(ValueError, match=r"lr_warmup_steps must be > 0 \(got %d\): the linear warm-up divides by it" % n):
        check_warmup(n)
    check_warmup(1)


def test_flatten_leaves_views_at_the_offsets():
    from causal_gen_amd.step_tail import Flat, flatten

    g = torch.Generator().manual_seed(0)
    ts = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((2, 3), (4,), (1, 1, 2))]
    want = [t.detach().clone() for t in ts]
    flat, offs = flatten(ts, "cpu")
    assert offs == [0, 6, 10] and flat.shape == (12,) and flat.dtype == torch.float32
    for t, w, o in zip(ts, want, offs):
        assert t.data_ptr() == flat.data_ptr() + 4 * o and t.shape == w.shape and torch.equal(t.detach(), w)
    flat.zero_()  # the parameters ARE the buffer
    assert not any(t.detach().any() for t in ts)
    f = Flat([("a", ts[0]), ("b", ts[1])], "cpu")
    assert f.names == ["a", "b"] and all(a is b for a, b in zip(f.params, ts)) and f.p_off == [0, 6] and f.flat_p.numel() == 10
