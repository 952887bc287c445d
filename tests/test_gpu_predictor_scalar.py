"""The train-mode scalar head on the MI355X: the kernel through the C ABI (cgen_mlp_train_fwd / _bwd) against the f64 oracle of
tests/predictor_scalar_ref.py, and ``PredictorTrainStep(scalar_heads=True)`` on a FlowPredictor -- loss and every gradient against
f64, the step against the f64 AdamW / EMA reference of tests/test_gpu_optim.py over the JOINT gradient, the EMA of encoder_a's
running statistics, capture, learning, the eval path, checkpoints, and that the default leaves encoder_a alone.

Bounds: the project's rule of tests/test_gpu_predictor_train.py.  Per tensor max|got - ref| / max|ref| <= max(bound, 4 e32) with
bound 1e-5 for the loss, 1e-4 for gradients, 1e-5 for running statistics, where e32 is the error of torch's own f32 CPU run against
the same f64 reference; every case asserts e32 <= 5e-5, so an ill-conditioned draw fails instead of widening a bound.  (n = 2 is
ill-conditioned by nature -- two rows normalise to +-1 whatever they were; torch's own e32 reaches 2e-4 there -- and gets a
runs-and-is-finite check only.)"""
import ctypes as C
import math
from types import SimpleNamespace

import pytest
import torch

import predictor_scalar_ref as S
import predictor_train_ref as R
from test_gpu_optim import U, f32, ref_update

from oracle import train_ref

pytestmark = pytest.mark.gpu

E32_MAX = 5e-5
BN = ("mlp.1", "mlp.4")


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Head:
    """One MLP on the device behind a cgen_mlp_train_head: its own gradient, workspace, terms and loss buffers"""

    def __init__(self, mlp, cols, strides, obs, obs_stride, n, tanh_loc=0, std_fixed=0.0, coef=1.0):
        from causal_gen_amd import _lib

        self.lib, self.n = _lib.require_gpu(), n
        self.mlp = mlp.cuda()
        self.P, self.B = dict(self.mlp.named_parameters()), dict(self.mlp.named_buffers())
        self.G = {k: torch.full_like(v, float("nan")) for k, v in self.P.items()}  # (overwritten, never accumulated into)
        r = self.rec = _lib.MlpTrainHead()
        r.nin, r.width, r.tanh_loc, r.std_fixed = len(cols), self.P["mlp.0.weight"].shape[0], tanh_loc, std_fixed
        for k, (p, s) in enumerate(zip(cols, strides)):
            r.in_[k], r.in_stride[k] = p, s
        r.obs, r.obs_stride = obs, obs_stride
        for i, name in enumerate(("mlp.0", "mlp.3", "mlp.6")):
            r.w[i], r.gw[i] = self.P[name + ".weight"].data_ptr(), self.G[name + ".weight"].data_ptr()
        r.bias, r.gb = self.P["mlp.6.bias"].data_ptr(), self.G["mlp.6.bias"].data_ptr()
        for i, name in enumerate(BN):
            r.gamma[i], r.beta[i] = self.P[name + ".weight"].data_ptr(), self.P[name + ".bias"].data_ptr()
            r.ggamma[i], r.gbeta[i] = self.G[name + ".weight"].data_ptr(), self.G[name + ".bias"].data_ptr()
            r.running_mean[i], r.running_var[i] = self.B[name + ".running_mean"].data_ptr(), self.B[name + ".running_var"].data_ptr()
            r.num_batches_tracked[i] = self.B[name + ".num_batches_tracked"].data_ptr()
        need = _lib.i64(0)
        self.lib.mlp_train_workspace(C.byref(r), n, C.byref(need))
        self.ws = torch.full((need.value,), float("nan"), device="cuda")
        self.terms = torch.full((n,), float("nan"), device="cuda")
        self.loss = torch.zeros(1, device="cuda")  # (the forward ADDS the sum of its terms)
        self.coef = torch.full((1,), coef, device="cuda")

    def run(self):
        st = torch.cuda.current_stream().cuda_stream
        self.lib.mlp_train_fwd(C.byref(self.rec), self.n, self.ws.data_ptr(), self.ws.numel(), S.MOMENTUM, self.terms.data_ptr(),
                               self.loss.data_ptr(), st)
        self.lib.mlp_train_bwd(C.byref(self.rec), self.n, self.ws.data_ptr(), self.ws.numel(), self.coef.data_ptr(), st)
        torch.cuda.synchronize()


def _dense_head(tag, coef=1.0):
    mlp, inp, obs, r64, e32 = S.reference(tag)
    _, _, n, _, std_fixed, tanh_loc, _ = S.CASES[tag]
    import copy

    cols = inp.t().contiguous().cuda()  # one buffer per column, row stride 1
    o = obs.cuda()
    hd = _Head(copy.deepcopy(mlp), [cols[k].data_ptr() for k in range(cols.shape[0])], [1] * cols.shape[0], o.data_ptr(), 1, n, tanh_loc,
               std_fixed, coef)
    hd.keep = (cols, o)
    return hd, r64, e32


def _compare(tag, hd, r64, e32):
    bad = {k: v for k, v in e32.items() if not v <= E32_MAX}
    assert not bad, f"case {tag}: ill-conditioned draw, torch f32 itself misses f64 by {bad}"
    errs = {"loss": abs(float(hd.loss) - float(r64["loss"])) / max(1.0, abs(float(r64["loss"])))}
    bounds = {"loss": max(1e-5, 4 * e32["loss"])}
    for n, ref in r64["grads"].items():
        errs[n], bounds[n] = R.rel_err(hd.G[n], ref), max(1e-4, 4 * e32[n])
    for n, ref in r64["bufs"].items():
        errs[n], bounds[n] = R.rel_err(hd.B[n], ref), max(1e-5, 4 * e32[n])
    for n in errs:
        print(f"case {tag} {n}: err {errs[n]:.3e} bound {bounds[n]:.3e} (torch f32 {e32[n]:.3e})")
    miss = {n: (errs[n], bounds[n]) for n in errs if not errs[n] <= bounds[n]}
    assert not miss, (tag, miss)
    assert abs(float(hd.terms.double().sum()) - float(r64["loss"])) <= bounds["loss"] * max(1.0, abs(float(r64["loss"])))
    for n in S.COUNTS:
        assert int(hd.B[n]) == int(r64["counts"][n]) == 1, n


@pytest.mark.parametrize("tag", sorted(S.CASES))
def test_kernel_matches_f64(tag):
    hd, r64, e32 = _dense_head(tag)
    hd.run()
    _compare(tag, hd, r64, e32)
    if tag == "std_fixed":
        assert float(hd.G["mlp.6.weight"][1].abs().max()) == 0.0 and float(hd.G["mlp.6.bias"][1]) == 0.0


def test_kernel_gradients_carry_the_coefficient():
    hd, r64, e32 = _dense_head("n5", coef=-0.25)
    hd.run()
    for n, ref in r64["grads"].items():
        assert R.rel_err(hd.G[n], -0.25 * ref) <= max(1e-4, 4 * e32[n]), n


def test_kernel_reads_strided_columns_of_a_wider_table():
    """inputs and target in place out of one [n, 5] table and one [n, 2] table: row strides 5, 2 and (a dense column) 1"""
    tag = "nin3_w64"
    mlp, inp, obs, r64, e32 = S.reference(tag)
    import copy

    n = inp.shape[0]
    wide = torch.full((n, 5), float("nan"))
    wide[:, 3], wide[:, 0] = inp[:, 0], inp[:, 2]
    pair = torch.full((n, 2), float("nan"))
    pair[:, 1], pair[:, 0] = inp[:, 1], obs[:, 0]
    wide, pair, dense = wide.cuda(), pair.cuda(), inp[:, 2].contiguous().cuda()
    # column 0 from the wide table (stride 5), column 1 from the pair (stride 2), column 2 dense (stride 1); target: pair's column 0
    hd = _Head(copy.deepcopy(mlp), [wide.data_ptr() + 12, pair.data_ptr() + 4, dense.data_ptr()], [5, 2, 1], pair.data_ptr(), 2, n)
    hd.run()
    _compare(tag + " strided", hd, r64, e32)
    ref, _, _ = _dense_head(tag)
    ref.run()
    for k in hd.G:  # the same numbers from the same values, wherever they lie
        assert torch.equal(_bits(hd.G[k]), _bits(ref.G[k])), k
    assert torch.equal(_bits(hd.loss), _bits(ref.loss))


def test_kernel_reruns_are_bit_identical():
    runs = []
    for _ in range(2):
        hd, _, _ = _dense_head("n257")
        hd.run()
        runs.append(hd)
    a, b = runs
    assert torch.equal(_bits(a.loss), _bits(b.loss)) and torch.equal(_bits(a.terms), _bits(b.terms))
    for k in a.G:
        assert torch.equal(_bits(a.G[k]), _bits(b.G[k])), k
    for k in S.STATS:
        assert torch.equal(_bits(a.B[k]), _bits(b.B[k])), k


def test_kernel_two_rows_run_and_stay_finite():
    from causal_gen_amd.predictor import MLP
    from predictor_ref import randomise

    g = torch.Generator().manual_seed(0)
    mlp = MLP(2, 32, 2)
    randomise(mlp, g)
    cols, obs = (torch.rand(2, 2, generator=g) * 1.6 - 0.8).cuda(), (torch.rand(2, 1, generator=g) * 1.6 - 0.8).cuda()
    hd = _Head(mlp, [cols[0].data_ptr(), cols[1].data_ptr()], [1, 1], obs.data_ptr(), 1, 2)
    hd.run()
    assert bool(torch.isfinite(hd.loss).all()) and bool(torch.isfinite(hd.terms).all())
    assert all(bool(torch.isfinite(v).all()) for v in hd.G.values()) and all(bool(torch.isfinite(hd.B[k]).all()) for k in S.STATS)


def test_forward_adds_its_sum_to_the_loss_already_there():
    hd, r64, e32 = _dense_head("n5")
    hd.loss.fill_(3.0)
    hd.run()
    assert abs(float(hd.loss) - 3.0 - float(r64["loss"])) <= max(1e-5, 4 * e32["loss"]) * max(1.0, abs(float(r64["loss"])))


# ------------------------------------------------------------------------------------------- the step on a FlowPredictor
def _step_cls():
    from causal_gen_amd.predictor_train import PredictorTrainStep

    return PredictorTrainStep


def _fresh(tag="e", **kw):
    pred, obs = R.make_case(tag)
    kw.setdefault("scalar_heads", True)
    return _step_cls()(pred, **kw), pred, obs


def test_step_loss_and_gradients_match_f64():
    pred, obs, r64, e32 = S.full_reference("e")
    bad = {k: v for k, v in e32.items() if not v <= E32_MAX}
    assert not bad, f"ill-conditioned draw, torch f32 itself misses f64 by {bad}"
    import copy

    pred = copy.deepcopy(pred)
    ts = _step_cls()(pred, ema=False, use_graph=False, scalar_heads=True)
    loss, grads = ts.loss_and_grads(**obs)
    assert set(grads) == set(r64["grads"]) == {n for n, _ in pred.named_parameters()}
    assert ts._on.names[-8:] == ["encoder_a." + n for n in S.PARAMS]  # (appended after the image heads')
    errs = {"loss": abs(float(loss) - float(r64["loss"])) / max(1.0, abs(float(r64["loss"])))}
    bounds = {"loss": max(1e-5, 4 * e32["loss"])}
    for n, ref in r64["grads"].items():
        errs[n], bounds[n] = R.rel_err(grads[n], ref), max(1e-4, 4 * e32[n])
    sd = pred.state_dict()
    for n, ref in r64["bufs"].items():
        errs[n], bounds[n] = R.rel_err(sd[n], ref), max(1e-5, 4 * e32[n])
    for n in errs:
        if n.startswith("encoder_a") or n == "loss":
            print(f"{n}: err {errs[n]:.3e} bound {bounds[n]:.3e} (torch f32 {e32[n]:.3e})")
    miss = {n: (errs[n], bounds[n]) for n in errs if not errs[n] <= bounds[n]}
    assert not miss, miss
    for n, ref in r64["counts"].items():
        assert int(sd[n]) == int(ref) == 1, n
    with pytest.raises(KeyError, match="age"):
        ts.loss_and_grads(**{k: v for k, v in obs.items() if k != "age"})


@pytest.mark.parametrize("clip", (200.0, 0.05), ids=("clip200", "clip_active"))
def test_step_is_the_joint_gradient_plus_the_optimiser_tail(clip):
    hp = SimpleNamespace(lr=f32(1e-4), betas=[f32(0.9), f32(0.999)], wd=f32(0.1), ema_rate=f32(0.999), lr_warmup_steps=1)
    ts, pred, obs = _fresh(lr=hp.lr, wd=hp.wd, betas=hp.betas, ema_rate=hp.ema_rate, lr_warmup_steps=1, grad_clip=clip)
    on, ema = ts._on, ts._ema
    a0 = on.p_off[on.names.index("encoder_a.mlp.0.weight")]
    for t0 in range(3):
        b0 = {"p": on.flat_p.clone(), "m": ts.m.clone(), "v": ts.v.clone(), "ema": ema.flat_p.clone()}
        out = ts.step(**obs)
        torch.cuda.synchronize()
        b0["g"] = ts.flat_g.clone()
        s = ts.state.cpu().double().tolist()
        norm = float(b0["g"].double().norm())  # over the image heads' AND encoder_a's gradient
        assert float(b0["g"][a0:].double().norm()) > 0.0
        cref = train_ref.clip_coef(norm, clip)  # ONE coefficient, from the joint norm, for encoder_a's slice of ref_update too
        assert s[3] == 0.0 and s[4] == 0.0 and s[5] == t0 + 1.0, s
        assert abs(s[1] - norm) <= 1e-5 * norm and abs(s[2] - cref) <= 1e-5 * cref, (s[:3], norm, cref)
        # (this batch's norm is about 1.2e3: 200 clips it too, by 0.17; 0.05 by 4e-5)
        assert cref < 1.0 and float(out["grad_norm"]) == s[1]
        ref = ref_update(b0, t0, s[2], hp)
        got = {"p": on.flat_p, "m": ts.m, "v": ts.v, "ema": ema.flat_p}
        for k, (want, tol) in ref.items():
            err = (got[k].double() - want).abs()
            assert bool((err <= tol).all()), (t0, k, float((err / tol.clamp_min(1e-300)).max()))
    assert ts.stats()["opt_steps"] == 3
    assert not torch.equal(on.flat_p[a0:], b0["p"][a0:])  # encoder_a moved


def test_ema_of_encoder_a_running_statistics():
    after, rate = 1, f32(0.999)
    ts, pred, obs = _fresh(lr=1e-3, ema_update_after=after, ema_rate=rate)
    on, ema = ts._on, ts._ema
    lo = on.b_off[on.bnames.index("encoder_a.mlp.1.running_mean")]
    assert on.bnames[-4:] == ["encoder_a." + n for n in S.STATS] and lo + 4 * 32 == on.flat_b.numel()
    averaged = 0
    for t0 in range(6):
        e0 = ema.flat_b[lo:].clone()
        ts.step(**obs)
        torch.cuda.synchronize()
        p = on.flat_b[lo:].double()
        d = train_ref.ema_decay(t0, rate, after)
        if d is None:
            assert torch.equal(ema.flat_b[lo:], on.flat_b[lo:]), t0
            continue
        want = e0.double() - (e0.double() - p) * (1.0 - d)
        tol = 8 * U * (e0.double().abs() + p.abs())
        err = (ema.flat_b[lo:].double() - want).abs()
        assert bool((err <= tol).all()), (t0, float((err / tol.clamp_min(1e-300)).max()))
        averaged += int(not torch.equal(ema.flat_b[lo:], on.flat_b[lo:]))
    assert averaged >= 2
    sd, esd = pred.state_dict(), ts.ema_model.state_dict()
    for n in S.STATS:
        o = ema.b_off[ema.bnames.index("encoder_a." + n)]
        assert torch.equal(esd["encoder_a." + n], ema.flat_b[o:o + 32]), n
    for n in S.COUNTS:
        assert int(esd["encoder_a." + n]) == 0 and int(sd["encoder_a." + n]) == 6, n


def test_captured_steps_equal_eager_steps():
    res = {}
    for graph in (True, False):
        ts, pred, obs = _fresh(lr=1e-3, use_graph=graph, ema_update_after=0)
        losses = [ts.step(**obs)["loss"] for _ in range(3)]  # captured: one eager step, then two replays
        torch.cuda.synchronize()
        assert bool(ts._graphs) == graph
        sd = pred.state_dict()
        counts = torch.stack([sd["encoder_a." + n] for n in S.COUNTS]).float()
        res[graph] = dict(loss=torch.stack(losses), p=ts._on.flat_p, b=ts._on.flat_b, ep=ts._ema.flat_p, eb=ts._ema.flat_b, m=ts.m, v=ts.v,
                          state=ts.state, counts=counts)
    assert bool((res[True]["counts"] == 3).all())
    for k in res[True]:
        assert torch.equal(_bits(res[True][k]), _bits(res[False][k])), k


def _age_term(ts):
    """mean of the age terms of the step just run (the training forward's, at the parameters before its update)"""
    (ent,) = ts._statics.values()
    ((_, _, terms),) = ent["scalars"]
    return float(terms.mean())


def test_twenty_steps_lower_the_age_term_and_predict_sees_the_trained_head():
    ts, pred, obs = _fresh(lr=1e-2, ema_update_after=0)  # (the EMA averages from the first step on: it differs from the online model)
    ts.step(**obs)
    a0 = _age_term(ts)
    for _ in range(20):
        ts.step(**obs)
    a20 = _age_term(ts)
    print(f"age term {a0:.4f} -> {a20:.4f} after 20 steps")
    assert math.isfinite(a20) and a20 < a0
    cobs = {k: v.cuda() for k, v in obs.items()}
    for model in (pred, ts.ema_model):
        assert not model.encoder_a.training
        ctx = torch.cat([cobs["brain_volume"], cobs["ventricle_volume"]], dim=-1)
        want = model.encoder_a(ctx)[:, :1]  # the module's own eval forward on the current parameters
        assert torch.equal(model.predict(**cobs)["age"], want)
    assert not torch.equal(pred.predict(**cobs)["age"], ts.ema_model.predict(**cobs)["age"])


def test_state_dict_round_trip():
    ts, pred, obs = _fresh(lr=1e-3, ema_update_after=0)
    for _ in range(3):
        ts.step(**obs)
    sd = ts.state_dict()
    assert set(sd["model_state_dict"]) == set(pred.state_dict()) == set(sd["ema_model_state_dict"])
    assert ["encoder_a." + n for n in S.PARAMS] == sd["optimizer_state_dict"]["names"][-8:]
    fresh, _ = R.make_case("e", seed=9)
    ts2 = _step_cls()(fresh, lr=1e-3, ema_update_after=0, scalar_heads=True)
    ts2.load_state_dict(sd)
    for part in ("model_state_dict", "ema_model_state_dict"):
        for k, v in ts2.state_dict()[part].items():
            assert torch.equal(v, sd[part][k]), (part, k)
    la, lb = ts.step(**obs)["loss"], ts2.step(**obs)["loss"]
    torch.cuda.synchronize()
    assert torch.equal(_bits(la), _bits(lb)) and ts.it == ts2.it == 4
    for a, b in ((ts._on.flat_p, ts2._on.flat_p), (ts._on.flat_b, ts2._on.flat_b), (ts._ema.flat_p, ts2._ema.flat_p),
                 (ts._ema.flat_b, ts2._ema.flat_b), (ts.m, ts2.m), (ts.v, ts2.v), (ts.state, ts2.state)):
        assert torch.equal(_bits(a), _bits(b))
    with pytest.raises(ValueError, match="other parameters"):  # a checkpoint of the image heads alone names other parameters
        _step_cls()(R.make_case("e")[0], scalar_heads=False).load_state_dict(sd)


def test_default_leaves_encoder_a_untouched():
    ts, pred, obs = _fresh(lr=1e-2, scalar_heads=False, ema_update_after=0)
    before = {k: v.clone() for k, v in pred.state_dict().items() if k.startswith("encoder_a.")}
    assert len(before) == 8 + 6
    for _ in range(3):
        ts.step(**{k: v for k, v in obs.items() if k != "age"})  # (and "age" is no required observation)
    torch.cuda.synchronize()
    after = pred.state_dict()
    for k, v in before.items():
        assert torch.equal(v, after[k]) and (not v.is_floating_point() or torch.equal(_bits(v), _bits(after[k]))), k
    names = ts.state_dict()["optimizer_state_dict"]["names"]
    assert names and not [n for n in names if "encoder_a" in n]
    assert not [n for n in ts._on.bnames if "encoder_a" in n]


def test_a_predictor_without_scalar_heads_is_bit_identical_either_way():
    res = {}
    for flag in (True, False):
        pred, obs = R.make_case("d")  # MorphoMNISTPredictor, R = 32, B = 5
        assert pred._scalar_heads() == []
        ts = _step_cls()(pred, lr=1e-3, ema_update_after=0, scalar_heads=flag)
        losses = [ts.step(**obs)["loss"] for _ in range(3)]
        torch.cuda.synchronize()
        res[flag] = dict(loss=torch.stack(losses), p=ts._on.flat_p, b=ts._on.flat_b, ep=ts._ema.flat_p, eb=ts._ema.flat_b, m=ts.m, v=ts.v,
                         state=ts.state, names=ts._on.names)
    assert res[True].pop("names") == res[False].pop("names")
    for k in res[True]:
        assert torch.equal(_bits(res[True][k]), _bits(res[False][k])), k
