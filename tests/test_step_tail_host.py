"""step_tail.StepTail without a GPU: CPU tensors and a stub library that records every call.  The launch sequence and every field of
every ``AdamwArgs`` are compared with lists written out here from what the three training steps issued before they shared the tail
(TrainStep: one adamw_ema per used range; PredictorTrainStep: the whole buffer, then the running statistics with lr = wd = 0 on a
zero gradient; PgmTrainStep: the whole buffer, 64 partial sums, no norm threshold).  Also ``check_warmup`` and ``flatten``, and the
supervised steps' skeleton ``SupStep`` as a toy subclass on CPU tensors: what ``_run`` issues in which order with a recorder in place
of ``capture``, what ``_optim`` hands to the tail, the checkpoint hooks, ``normalize_columns`` and ``check_index``."""
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


def _toy(monkeypatch, use_graph=True, ema=True, regions=None):
    """A SupStep on CPU tensors: the stub library, a recorder in place of ``capture`` and a log of what ran, in order."""
    from causal_gen_amd import step_tail

    lib, log = StubLib(), []
    monkeypatch.setattr(step_tail._lib, "require_gpu", lambda: lib)

    class Graph:
        def replay(self):
            log.append("replay")

    def capture(fn):
        log.append("capture")
        return Graph(), fn()

    monkeypatch.setattr(step_tail, "capture", capture)

    class ToyFlat(step_tail.Flat):
        def invalidate(self):
            log.append(("flat.invalidate", self.which))

    class Toy(step_tail.SupStep):
        NORM_BLOCKS = 8

        def _flatten(self, model, dev):
            f = ToyFlat(model.named_parameters(), dev)
            f.which = "online" if model is net else "ema"
            log.append(("flatten", f.which))
            return f

        def _stream(self):
            return ST

        def _fwd_bwd(self, ent):
            log.append(("fwd_bwd", ent))

        def _optim(self):
            log.append("optim")
            super()._optim()

        def _invalidate(self):
            log.append("_invalidate")
            super()._invalidate()

    if regions is not None:
        Toy._ema_only = lambda self: regions
    net = torch.nn.Linear(3, 2)
    ts = Toy(net, lr=1e-4, wd=0.1, betas=(0.9, 0.999), eps=1e-8, grad_clip=200.0, lr_warmup_steps=1, ema_rate=0.999, ema=ema,
             use_graph=use_graph, ema_update_after=100, device="cpu")
    return ts, lib, log


def test_sup_step_builds_the_shared_middle(monkeypatch):
    from causal_gen_amd.step_tail import HyperParams

    ts, lib, log = _toy(monkeypatch)
    assert log == [("flatten", "ema"), ("flatten", "online")]  # the EMA copy first, the online model second
    assert ts.hp == HyperParams(1e-4, (0.9, 0.999), 1e-8, 0.1, 200.0, float("inf"), 1, 0.999, 100) and not ts.hp.const_lr
    assert ts.ema_model is not ts.model and not any(p.requires_grad for p in ts.ema_model.parameters())
    assert ts._on.names == ts._ema.names == ["weight", "bias"] and ts._on.flat_p.numel() == 8
    assert ts.flat_g.shape == (8,) and not ts.flat_g.any() and ts.tail.norm_blocks == 8 and ts.tail.lib is lib
    assert ts.m is ts.tail.m and ts.v is ts.tail.v and ts.state is ts.tail.state and ts.partial is ts.tail.partial
    assert ts.stats == ts.tail.stats and ts.out3.shape == (3,) and ts.res.shape == (2,)
    assert ts._statics == {} and ts._graphs == {} and ts.it == 0
    no_ema, _, _ = _toy(monkeypatch, ema=False)
    assert no_ema.ema_model is None and no_ema._ema is None
    with pytest.raises(ValueError, match="lr_warmup_steps must be > 0"):
        type(ts)(torch.nn.Linear(3, 2), lr=1e-4, wd=0.1, betas=(0.9, 0.999), eps=1e-8, grad_clip=200.0, lr_warmup_steps=0, ema_rate=0.999,
                 ema=True, use_graph=True, ema_update_after=100, device="cpu")


def test_sup_step_run_is_eager_then_captured_then_replayed(monkeypatch):
    ts, lib, log = _toy(monkeypatch)
    del log[:]
    inval = ["_invalidate", ("flat.invalidate", "online"), ("flat.invalidate", "ema")]
    ts.state[1] = 2.5  # (NORM: what the tail's kernels would have left)
    ts.res[0] = 7.0
    out = ts._run("k", "ent")
    assert log == [("fwd_bwd", "ent"), "optim", "capture", ("fwd_bwd", "ent"), "optim"] + inval  # eager body, captured body, invalidate
    assert sorted(out) == ["grad_norm", "loss"] and float(out["loss"]) == 7.0 and float(out["grad_norm"]) == 2.5
    assert out["loss"].data_ptr() != ts.res.data_ptr()  # a copy: the next step does not change what the caller holds
    del log[:]
    ts._run("k", "ent")
    assert log == ["replay"] + inval
    del log[:]
    ts._run("other", "ent2")  # another key is another eager step and another graph
    assert log[:3] == [("fwd_bwd", "ent2"), "optim", "capture"] and sorted(ts._graphs) == ["k", "other"]
    assert ts.it == 3
    assert [c[0] for c in lib.calls] == ["sumsq_partial", "clip_decide", "adamw_ema", "step_commit"] * 4  # one tail per body


def test_sup_step_without_a_graph_never_captures(monkeypatch):
    ts, _, log = _toy(monkeypatch, use_graph=False, ema=False)
    del log[:]
    for _ in range(3):
        ts._run("k", "ent")
    assert log == [("fwd_bwd", "ent"), "optim", "_invalidate", ("flat.invalidate", "online")] * 3
    assert ts._graphs == {} and ts.it == 3


def test_sup_step_optim_passes_the_ema_only_regions_through(monkeypatch):
    pb, eb = torch.ones(7), torch.ones(7)
    ts, lib, _ = _toy(monkeypatch, regions=[(pb.data_ptr(), eb.data_ptr(), 7)])
    ts._optim()
    S = ts.state.data_ptr()
    assert [c[0] for c in lib.calls] == ["sumsq_partial", "clip_decide", "adamw_ema", "adamw_ema", "step_commit"]
    assert lib.calls[0] == ("sumsq_partial", (ts.flat_g.data_ptr(), 8, ts.partial.data_ptr(), 8, ST))
    assert lib.calls[1] == ("clip_decide", (ts.partial.data_ptr(), 8, ts.out3.data_ptr(), 200.0, float("inf"), S, ST))
    assert lib.calls[2] == ("adamw_ema", (_args(ts._on.flat_p.data_ptr(), ts.flat_g.data_ptr(), ts.m.data_ptr(), ts.v.data_ptr(),
                                                ts._ema.flat_p.data_ptr(), 8, S, lr=1e-4, wd=0.1, beta2=0.999, warmup=1), ST))
    q, st = lib.calls[3][1]
    assert (q["p"], q["ema"], q["count"], q["lr"], q["wd"], st) == (pb.data_ptr(), eb.data_ptr(), 7, 0.0, 0.0, ST)
    plain, lib2, _ = _toy(monkeypatch, ema=False)  # the default hook: no region; no EMA copy: no ema pointer
    plain._optim()
    assert [c[0] for c in lib2.calls] == ["sumsq_partial", "clip_decide", "adamw_ema", "step_commit"] and lib2.calls[2][1][0]["ema"] is None


def test_sup_step_checkpoint_keys_and_hooks(monkeypatch):
    ts, _, log = _toy(monkeypatch)
    assert list(ts.state_dict()) == ["step", "model_state_dict", "optimizer_state_dict", "ema_model_state_dict"]
    type(ts)._extra_state = lambda self: {"rng_state": 5}
    ts.it, ts.m[0] = 4, 3.0
    sd = ts.state_dict()
    assert list(sd) == ["step", "model_state_dict", "optimizer_state_dict", "rng_state", "ema_model_state_dict"]
    other, _, log2 = _toy(monkeypatch)  # (a class of its own)
    type(other)._load_extra_state = lambda self, sd: log2.append(("extra", sd["rng_state"]))
    del log2[:]
    other.load_state_dict(sd)
    assert other.it == 4 and torch.equal(other.m, ts.m) and torch.equal(other._on.flat_p, ts._on.flat_p)
    assert torch.equal(other._ema.flat_p, ts._ema.flat_p) and other.model.weight.data_ptr() == other._on.flat_p.data_ptr()
    assert log2 == [("extra", 5), "_invalidate", ("flat.invalidate", "online"), ("flat.invalidate", "ema")]  # extras, then it, invalidate
    with pytest.raises(KeyError):  # by default a checkpoint without an optimiser state is an error
        other.load_state_dict({k: v for k, v in sd.items() if k != "optimizer_state_dict"})
    type(other)._optimizer_state = lambda self, sd: sd.get("optimizer_state_dict")
    other.load_state_dict({k: v for k, v in sd.items() if k != "optimizer_state_dict"})


def test_normalize_columns_and_check_index():
    from causal_gen_amd.step_tail import check_index, normalize_columns

    assert normalize_columns({"a": 3, "b": (4, 2)}) == {"a": (3, 1), "b": (4, 2)}
    assert normalize_columns(None) is None
    bad = {"int32": torch.zeros(4, dtype=torch.int32), "two-dimensional": torch.zeros(2, 2, dtype=torch.int64),
           "host": torch.zeros(4, dtype=torch.int64)}
    for what, index in bad.items():
        with pytest.raises(ValueError, match=r"^Some\.step_from: the index must be a device int64 vector$"):
            check_index(index, "Some.step_from")
    if torch.cuda.is_available():  # (dtype and rank are what is refused above, not only the host)
        check_index(torch.zeros(4, dtype=torch.int64, device="cuda"), "Some.step_from")
        for what in ("int32", "two-dimensional"):
            with pytest.raises(ValueError, match="Some.step_from"):
                check_index(bad[what].cuda(), "Some.step_from")
