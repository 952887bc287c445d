"""Counterfactual evaluation on the GPU: cgen_metric_accum, cgen_rocauc and cgen_image_dist against the f64 references of
tests/cf_eval_ref.py, graph capture, and CfEvaluator / predictor_eval against the same references applied to predictor.predict()."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_golden
import cf_eval_ref as R
from predictor_ref import randomise

pytestmark = pytest.mark.gpu


def _ulps(got, want):
    """|got - want| in units of want's f32 spacing."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def _same(a, b, tol=0.0):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= tol


def _specs():
    from causal_gen_amd.cf_eval import MetricSpec

    return [MetricSpec("bs", "binary", 1, "sigmoid", ("rocauc", "acc")), MetricSpec("bn", "binary", 1, "none", ("rocauc", "acc")),
            MetricSpec("cs", "categorical", 10, "softmax", ("acc", "rocauc")), MetricSpec("cn", "categorical", 3, "none", ("acc", "rocauc")),
            MetricSpec("rn", "continuous", 1, "none", ("mae",), 392953.5, 1235719.5, 392953.5, 1235719.5, 1000.0),
            MetricSpec("rt", "continuous", 1, "tanh", ("mae",), 2.5, 3.5, 2.5, 3.5, 1.0)]


def _batch(g, n, specs):
    """One batch of raw predictions / targets ({name: [n, ncls]} f32 CPU), logits drawn with |o| >= 1e-3."""
    away = lambda shape: (torch.randint(0, 2, shape, generator=g).float() * 2 - 1) * (1e-3 + 2.0 * torch.randn(shape, generator=g).abs())
    p, t = {}, {}
    for s in specs:
        if s.kind == "binary":
            o = away((n, 1))
            p[s.name] = o if s.transform == "sigmoid" else (0.5 + o.clamp(-4, 4) / 8.1)  # probabilities, |p - 0.5| >= 1e-4
            t[s.name] = torch.randint(0, 2, (n, 1), generator=g).float()
        elif s.kind == "categorical":
            o = 2.0 * torch.randn(n, s.ncls, generator=g)
            p[s.name] = o if s.transform == "softmax" else torch.softmax(o, -1)
            t[s.name] = torch.nn.functional.one_hot(torch.randint(0, s.ncls, (n,), generator=g), s.ncls).float()
        else:
            p[s.name] = away((n, 1))
            t[s.name] = torch.rand(n, 1, generator=g) * 2 - 1
    return p, t


def _special(p, t, specs, row, what):
    for s in specs:
        if what == "zero" and s.kind == "binary" and s.transform == "sigmoid":
            p[s.name][row, 0] = 0.0  # round(sigmoid(0)) = round(0.5) = 0: predicted class 0
        elif what == "nan_pred":
            p[s.name][row, s.ncls - 1] = float("nan")
        elif what == "inf_target":
            t[s.name][row, 0] = float("inf")


def _laid_out(v, stride):
    """[n, k] CPU rows -> a CUDA view with row stride max(stride, k) (the rest of each row is poison the kernel must not read)."""
    n, k = v.shape
    if stride <= k:
        return v.cuda().contiguous()
    buf = torch.full((n, stride), float("nan"), device="cuda")
    buf[:, :k] = v.cuda()
    return buf[:, :k]


@pytest.mark.parametrize("n", [1, 3, 64, 257])
@pytest.mark.parametrize("pred_stride,target_stride", [(1, 1), (16, 10)])
def test_metric_accum_against_f64(n, pred_stride, target_stride):
    from causal_gen_amd import cf_eval

    specs = _specs()
    g = torch.Generator().manual_seed(100 + n)
    batches = [_batch(g, n, specs) for _ in range(3)]
    if n >= 3:
        _special(*batches[0], specs, 0, "zero")
        _special(*batches[1], specs, n - 1, "nan_pred")
        _special(*batches[2], specs, n // 2, "inf_target")
    else:  # too few rows to hold the special ones: three more one-row updates
        for what in ("zero", "nan_pred", "inf_target"):
            b = _batch(g, 1, specs)
            _special(*b, specs, 0, what)
            batches.append(b)
    acc = cf_eval.MetricAccumulator(specs, capacity=1024)
    dev_in = []
    for p, t in batches:
        dp = {k: _laid_out(v, pred_stride) for k, v in p.items()}
        dt = {k: _laid_out(v, target_stride) for k, v in t.items()}
        if pred_stride > 1:
            assert dp["bs"].stride(0) == 16 and dt["bs"].stride(0) == 10 and dt["cs"].stride(0) == 10
        dev_in.append((dp, dt))
        acc.update(dp, dt)
    got = acc.compute()
    allp = {k: torch.cat([b[0][k] for b in batches]).numpy() for k in batches[0][0]}
    allt = {k: torch.cat([b[1][k] for b in batches]).numpy() for k in batches[0][0]}
    total = sum(b[0]["bs"].shape[0] for b in batches)
    for i, s in enumerate(specs):
        if s.kind == "binary":
            want = R.binary_metrics(allp[s.name], allt[s.name], s.transform)
        elif s.kind == "categorical":
            want = R.categorical_metrics(allp[s.name], allt[s.name], s.ncls, s.transform)
        else:
            want = R.continuous_metrics(allp[s.name], allt[s.name], s.transform, s.pred_scale, s.pred_shift, s.tgt_scale, s.tgt_shift, s.norm)
        assert got["n_skipped"][s.name] == want["n_skipped"] == 2, (s.name, got["n_skipped"], want["n_skipped"])
        assert got["n"][s.name] == want["n"] == total - 2 and got["n_overflow"][s.name] == 0
        if s.kind == "continuous":
            print(s.name, "mae", got[s.name + "_mae"], want["mae"])
            assert abs(got[s.name + "_mae"] - want["mae"]) <= 1e-6 * abs(want["mae"]), (s.name, got[s.name + "_mae"], want["mae"])
            continue
        assert int(acc.acc[i, 1].item()) == want["correct"], (s.name, acc.acc[i, 1].item(), want["correct"])
        assert got[s.name + "_acc"] == want["acc"]
        rows = int(acc.row_count[i].item())
        assert rows == want["n"]
        sc, lb = acc.scores[s.name][:rows].cpu().numpy(), acc.labels[s.name][:rows].cpu().numpy()
        assert np.array_equal(lb.reshape(want["labels"].shape), want["labels"]), s.name
        # the stored scores against torch's own f32 transform of the kept rows, on the device
        keep = torch.from_numpy(R.finite_rows(allp[s.name], allt[s.name], s.ncls, s.ncls if s.kind == "categorical" else 1))
        raw = torch.from_numpy(allp[s.name])[keep][:, :s.ncls].cuda()
        ref32 = {"sigmoid": torch.sigmoid, "softmax": lambda v: torch.softmax(v, -1), "none": lambda v: v}[s.transform](raw).cpu().numpy()
        u = _ulps(sc.reshape(ref32.shape), ref32).max()
        print(s.name, "score ulps", u)
        assert u <= (2.0 if s.transform != "none" else 0.0), (s.name, u)
        assert np.abs(sc.reshape(want["scores"].shape) - want["scores"]).max() <= 3e-7  # and against the f64 transform
        want_auc = np.mean([R.auc_pairs(sc[:, c], lb[:, c]) for c in range(s.ncls)])  # the pair formula on the device's scores
        assert _same(got[s.name + "_rocauc"], want_auc, 1e-12), (s.name, got[s.name + "_rocauc"], want_auc)


def test_zero_logit_is_class_zero():
    from causal_gen_amd import cf_eval

    spec = [cf_eval.MetricSpec("s", "binary", 1, "sigmoid", ("acc",))]
    acc = cf_eval.MetricAccumulator(spec, capacity=0)
    acc.update({"s": torch.zeros(2, 1).cuda()}, {"s": torch.tensor([[0.0], [1.0]]).cuda()})
    got = acc.compute()
    assert got["n"]["s"] == 2 and got["s_acc"] == 0.5 and int(acc.acc[0, 1].item()) == 1


def test_score_buffer_overflow_drops_rows_from_the_auc_only():
    from causal_gen_amd import cf_eval

    spec = [cf_eval.MetricSpec("s", "binary", 1, "sigmoid", ("rocauc", "acc"))]
    acc = cf_eval.MetricAccumulator(spec, capacity=100)
    guard = 64
    big_s, big_l = torch.full((100 + guard,), -7.0, device="cuda"), torch.full((100 + guard,), -7.0, device="cuda")
    acc.scores["s"], acc.labels["s"] = big_s[:100].view(100, 1), big_l[:100].view(100, 1)
    g = torch.Generator().manual_seed(4)
    ps, ts = [], []
    for _ in range(3):
        p, t = _batch(g, 64, spec)
        ps.append(p["s"])
        ts.append(t["s"])
        acc.update({"s": p["s"].cuda()}, {"s": t["s"].cuda()})
    got = acc.compute()
    p, t = torch.cat(ps).numpy(), torch.cat(ts).numpy()
    full, first = R.binary_metrics(p, t), R.binary_metrics(p, t, capacity=100)
    assert got["n_overflow"]["s"] == 92 and got["n"]["s"] == 192 and got["n_skipped"]["s"] == 0
    assert got["s_acc"] == full["acc"] and int(acc.acc[0, 1].item()) == full["correct"]
    assert int(acc.row_count[0].item()) == 100
    sc, lb = big_s[:100].cpu().numpy(), big_l[:100].cpu().numpy()
    assert np.array_equal(lb, first["labels"]) and np.abs(sc - first["scores"]).max() <= 3e-7
    assert _same(got["s_rocauc"], R.auc_pairs(sc, lb), 1e-12)
    assert abs(got["s_rocauc"] - R.auc_pairs(first["scores"], first["labels"])) <= 1e-3  # (f32 scores may tie where f64 ones do not)
    assert bool((big_s[100:] == -7.0).all()) and bool((big_l[100:] == -7.0).all()), "the guard band after the score buffer was written"
    acc.reset()
    assert int(acc.row_count[0].item()) == 0 and float(acc.acc.abs().sum().item()) == 0.0


def _rocauc(scores, labels, n, ncls, stride, n_rows_max=None):
    """cgen_rocauc on CUDA [rows, stride] buffers whose device-side row count is n."""
    from causal_gen_amd import _lib

    lib = _lib.require_gpu()
    cnt = torch.tensor([n], dtype=torch.int64, device="cuda")
    out = torch.full((ncls,), -1.0, dtype=torch.float64, device="cuda")
    ws = torch.full((4 * ncls,), 12345, dtype=torch.int64, device="cuda")  # (the call zeroes it)
    lib.rocauc(scores.data_ptr(), labels.data_ptr(), cnt.data_ptr(), scores.shape[0] if n_rows_max is None else n_rows_max, ncls, stride,
               out.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return out.cpu().numpy()


@pytest.mark.parametrize("case", ["continuous", "four_levels", "all_equal", "separated", "three_columns"])
def test_rocauc_against_the_pair_formula(case):
    g = torch.Generator().manual_seed(11)
    for n in (2, 63, 64, 65, 1000, 4097):
        ncls, stride = (3, 16) if case == "three_columns" else (1, 1)
        rows = n + 300  # rows past the device-side count hold other data: the count is read on the device, not taken from n_rows_max
        lab = (torch.rand(rows, stride, generator=g) < 0.4).float()
        lab[0], lab[1] = 1.0, 0.0
        s = torch.randn(rows, stride, generator=g)
        if case == "four_levels":
            s = torch.floor(torch.rand(rows, stride, generator=g) * 4) / 4
        elif case == "all_equal":
            s = torch.full((rows, stride), 0.25)
        elif case == "separated":
            s = lab * 2.0 + torch.rand(rows, stride, generator=g)
        ds, dl = s.cuda(), lab.cuda()
        got = _rocauc(ds, dl, n, ncls, stride)
        back_s, back_l = ds.cpu().numpy().astype(np.float64), dl.cpu().numpy()
        for c in range(ncls):
            want = R.auc_pairs(back_s[:n, c], back_l[:n, c])
            assert abs(got[c] - want) <= 1e-12, (case, n, c, got[c], want)
            if case == "all_equal":
                assert got[c] == 0.5
            if case == "separated":
                assert got[c] == 1.0
        if n <= 1000:
            assert abs(got[0] - R.auc_pairs_brute(back_s[:n, 0], back_l[:n, 0])) <= 1e-12
        assert np.array_equal(got, _rocauc(ds, dl, n, ncls, stride)), "reruns are bit-identical"


def test_rocauc_with_a_class_absent_is_nan():
    s = torch.randn(70, 2).cuda()
    lab = torch.zeros(70, 2)
    lab[:, 1] = 1.0
    lab[3, 0] = 1.0
    lab[5, 1] = 0.0
    got = _rocauc(s, lab.cuda(), 70, 2, 2)
    assert not np.isnan(got).any()
    lab[3, 0], lab[5, 1] = 0.0, 1.0  # column 0 without a positive, column 1 without a negative
    got = _rocauc(s, lab.cuda(), 70, 2, 2)
    assert np.isnan(got).all()
    assert np.isnan(_rocauc(s, lab.cuda(), 0, 2, 2)).all()  # no rows at all


@pytest.mark.parametrize("shape", [(1, 1, 32, 32), (3, 3, 32, 32), (5, 1, 40, 24), (2, 1, 192, 192)])
def test_image_dist_against_f64(shape):
    """The kernel forms differences and sums in f64 throughout: the accumulated sums are held to 1e-12 relative; the per-image
    f32 outputs carry one rounding to f32 (2^-24 relative), held to 1e-7."""
    from causal_gen_amd import cf_eval

    g = torch.Generator().manual_seed(sum(shape))
    numel = int(np.prod(shape))
    flat_a, flat_b = torch.rand(numel + 1, generator=g) * 2 - 1, torch.rand(numel + 1, generator=g) * 2 - 1
    da, db = flat_a.cuda(), flat_b.cuda()
    views = {"aligned": (da[:numel].view(shape), db[:numel].view(shape), flat_a[:numel], flat_b[:numel]),
             "both_off_by_one": (da[1:].view(shape), db[1:].view(shape), flat_a[1:], flat_b[1:]),
             "one_off_by_one": (da[:numel].view(shape), db[1:].view(shape), flat_a[:numel], flat_b[1:])}
    for name, (a, b, ca, cb) in views.items():
        assert (a.data_ptr() % 16 == 0) == (name != "both_off_by_one") and (b.data_ptr() % 16 == 0) == (name == "aligned")
        acc = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64, device="cuda")
        per = cf_eval.image_distance(a, b, acc)
        want = R.image_dist(ca.numpy().reshape(shape), cb.numpy().reshape(shape))
        assert tuple(per.shape) == (shape[0], 2)
        rel = np.abs(per.cpu().numpy().astype(np.float64) - want) / want
        assert rel.max() <= 1e-7, (name, rel.max())
        got = acc.cpu().numpy() - np.array([1.0, 2.0, 3.0])
        assert got[2] == shape[0]
        assert np.abs(got[:2] - want.sum(0)).max() <= 1e-12 * want.sum(0).max(), (name, got, want.sum(0))
        same = cf_eval.image_distance(a, a.clone())
        assert float(same.abs().max()) == 0.0, name


def test_update_and_image_distance_captured_in_a_graph():
    """One eager call, capture, two replays == three eager calls, bit for bit."""
    from causal_gen_amd import cf_eval

    specs = _specs()
    g = torch.Generator().manual_seed(21)
    p, t = _batch(g, 70, specs)
    p, t = {k: v.cuda() for k, v in p.items()}, {k: v.cuda() for k, v in t.items()}
    a, b = torch.rand(3, 1, 40, 24, generator=g).cuda(), torch.rand(3, 1, 40, 24, generator=g).cuda()

    eager = cf_eval.MetricAccumulator(specs, capacity=150)
    eager_d = torch.zeros(3, dtype=torch.float64, device="cuda")
    for _ in range(3):
        eager.update(p, t)
        eager_per = cf_eval.image_distance(a, b, eager_d)

    graphed = cf_eval.MetricAccumulator(specs, capacity=150)
    graphed_d = torch.zeros(3, dtype=torch.float64, device="cuda")
    graphed.update(p, t)
    cf_eval.image_distance(a, b, graphed_d)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, capture_error_mode="thread_local"):
        graphed.update(p, t)
        per = cf_eval.image_distance(a, b, graphed_d)
    gr.replay()
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(graphed.acc, eager.acc) and torch.equal(graphed.row_count, eager.row_count)
    assert int(eager.row_count[0].item()) == 150 and float(eager.acc[0, 4].item()) == 60.0  # 3 x 70 rows into 150
    for k in eager.scores:
        assert torch.equal(graphed.scores[k], eager.scores[k]) and torch.equal(graphed.labels[k], eager.labels[k]), k
    assert torch.equal(graphed_d, eager_d) and torch.equal(per, eager_per)
    r0, r1 = eager.compute(), graphed.compute()
    assert repr(r0) == repr(r1)


# ----------------------------------------------------------------------------- model level
def _targets(cf_pa, do):
    return {k: (do[k] if k in do else v) for k, v in cf_pa.items()}


def _check_effectiveness(ev, pred, scm, pa, dos, imgs, res, specs_pred):
    """The evaluator's numbers against the reference metrics applied to predictor.predict() on the returned images."""
    for name, do in dos.items():
        cf_pa = scm.counterfactual(obs=pa, intervention=do, num_particles=1)
        preds = pred.predict(x=imgs[name], **cf_pa)
        tg = _targets(cf_pa, do)
        got = res[name]
        for s in specs_pred:
            want = R.spec_metrics(s, preds[s.name].detach().cpu().numpy(), tg[s.name].detach().cpu().numpy())
            assert got["n"][s.name] == want["n"] == imgs[name].shape[0] and got["n_skipped"][s.name] == 0
            for m in s.metrics:
                key = s.name + "_" + m
                print(name, key, got[key], want[key])
                if m == "mae":
                    assert abs(got[key] - want[key]) <= 1e-6 * abs(want[key]), (name, key, got[key], want[key])
                elif m == "acc":
                    assert got[key] == want[key], (name, key, got[key], want[key])
                else:  # B rows: few distinct pairs, any disagreement is a whole pair
                    assert _same(got[key], want[key], 1e-12), (name, key, got[key], want[key])


def _replayed_images(vae, ev, x, pa, scm, dos, rng_before):
    """cf_pixels(x, rec, forward_latents(zs, cf_pa_k)) from the SAME zs: the Philox state is put back to where the evaluator
    found it, so the abduction draws the same noise."""
    from causal_gen_amd import dscm

    eng = vae.engine()
    eng.rng.copy_(rng_before)
    zs, (rec_loc, rec_scale) = vae.abduct_with_reconstruction(x, ev._pre(pa), t=ev.t_abduct)
    if vae.cond_prior:
        zs = [z["z"] for z in zs]
    out = {}
    for name, do in dos.items():
        cf_pa = scm.counterfactual(obs=pa, intervention=do, num_particles=1)
        cf_loc, cf_scale = vae.forward_latents(zs, ev._pre(cf_pa))
        out[name] = dscm.cf_pixels(x, rec_loc, rec_scale, cf_loc, cf_scale)
    return out


def _rng_state(vae):
    eng = vae.engine()
    eng.rng_ptr()
    return eng.rng.clone()


@pytest.fixture(scope="module")
def morpho():
    from causal_gen_amd import pgm, predictor as P, vae
    from causal_gen_amd.hps import setup_hparams
    from oracle import fullsize_recipe as FR

    hp = setup_hparams("morphomnist", cond_prior=False)
    hp.dataset = "morphomnist"
    torch.manual_seed(7)
    m = vae.HVAE(hp)
    m.apply(FR.init_bias)
    FR.perturb(m)
    m.compute_dtype = "f32"
    m = m.cuda().eval()
    g = torch.Generator().manual_seed(3)
    scm = pgm.MorphoMNISTPGM(SimpleNamespace(widths=[8, 8]))
    with torch.no_grad():
        for p in scm.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.5)
    scm = scm.cuda()
    pred = P.MorphoMNISTPredictor(SimpleNamespace(input_channels=1, input_res=32, std_fixed=0.0))
    randomise(pred, g)
    pred = pred.cuda()
    B = 4
    pa = scm.sample(B, torch.Generator().manual_seed(5))
    x = ((torch.randint(0, 256, (B, 1, 32, 32), generator=g).float() - 127.5) / 127.5).cuda()
    return hp, m, scm, pred, pa, x


def test_effectiveness_on_the_morphomnist_preset(morpho):
    from causal_gen_amd import cf_eval

    hp, m, scm, pred, pa, x = morpho
    B = x.shape[0]
    mm = {"thickness": (0.5, 7.5), "intensity": (60.0, 255.0)}
    ev = cf_eval.CfEvaluator(m, scm, pred, hp, capacity=64, min_max=mm)
    dos = {"do(thickness)": {"thickness": pa["thickness"].roll(1, 0)}, "do(intensity)": {"intensity": -0.5 * pa["intensity"]},
           "do(digit)": {"digit": pa["digit"].roll(1, 0)}, "null": {}}
    rng = _rng_state(m)
    obs = dict(pa, x=x)
    imgs = ev.effectiveness(obs, list(dos.values()), return_images=True)
    assert list(imgs) == list(dos)
    res = ev.results()["effectiveness"]
    _check_effectiveness(ev, pred, scm, pa, dos, imgs, res, cf_eval.metric_specs("morphomnist", mm, raw=False))
    want = _replayed_images(m, ev, x, pa, scm, dos, rng)
    for k in dos:
        assert torch.equal(imgs[k], want[k]), k
    assert not torch.equal(imgs["do(thickness)"], imgs["null"])
    # a second batch accumulates: twice the rows, the same accuracy
    ev.effectiveness(obs, list(dos.values()))
    again = ev.results()["effectiveness"]
    assert again["null"]["n"]["digit"] == 2 * B


def test_composition_and_reversibility_on_the_morphomnist_preset(morpho):
    from causal_gen_amd import cf_eval

    hp, m, scm, pred, pa, x = morpho
    ev = cf_eval.CfEvaluator(m, scm, pred, hp, capacity=64)
    obs = dict(pa, x=x)
    per = ev.composition(obs, cycles=2)
    assert len(per) == 2 and tuple(per[0].shape) == (x.shape[0], 2)
    rev = ev.reversibility(obs, {"thickness": pa["thickness"].roll(1, 0)}, cycles=1)
    out = ev.results()
    comp1 = out["composition"][1]
    print("composition", out["composition"], "reversibility", out["reversibility"])
    # the bound of test_gpu_train.test_full_size_null_intervention_returns_the_observation, on the [-1, 1] scale
    assert float(per[0][:, 0].max()) < 1e-5 and comp1["l1"] < 1e-5 and comp1["n"] == x.shape[0]
    assert comp1["l1_grey"] == comp1["l1"] * 127.5
    assert abs(comp1["l1"] - float(per[0][:, 0].double().mean())) <= 1e-6 * comp1["l1"] + 1e-12
    r1 = out["reversibility"][1]
    assert r1["n"] == x.shape[0] and np.isfinite(r1["l1"]) and r1["l2"] >= 0.0
    assert abs(r1["l1"] - float(rev[0][:, 0].double().mean())) <= 1e-6 * r1["l1"] + 1e-12
    assert r1["l1"] > 0.0  # (a fresh abduction per hop: the round trip is close to, not equal to, the observation)


def test_effectiveness_on_the_ukbb_light_fixture_with_the_host_side_age_head():
    from causal_gen_amd import cf_eval, pgm, predictor as P, vae
    from causal_gen_amd.hps import Hparams

    fx = load_golden("dscm_ukbb_light_p1.pt")
    hpd = dict(fx["hp"])
    m = vae.HVAE(Hparams(**hpd))
    m.load_state_dict(fx["state_dict"])
    m.compute_dtype = "f32"
    m = m.cuda().eval()
    args = SimpleNamespace(**{**hpd, "parents_x": fx["parents_x"], "dataset": fx["dataset"]})
    g = torch.Generator().manual_seed(1)
    scm = pgm.FlowPGM(SimpleNamespace(widths=[8, 8]))
    with torch.no_grad():
        for p in scm.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.5)
    scm = scm.cuda()
    pred = P.FlowPredictor(SimpleNamespace(input_channels=1, input_res=16, std_fixed=0.0))
    randomise(pred, g)
    pred = pred.cuda()
    B = 4
    pa = scm.sample(B, torch.Generator().manual_seed(2))
    x = ((torch.randint(0, 256, (B, 1, 16, 16), generator=g).float() - 127.5) / 127.5).cuda()
    assert pred.path(x) == "fused"
    ev = cf_eval.CfEvaluator(m, scm, pred, args, capacity=32)
    assert [s.name for s in ev.specs] == ["sex", "mri_seq", "age", "brain_volume", "ventricle_volume"]
    dos = {"do(sex)": {"sex": 1 - pa["sex"]}, "do(age)": {"age": pa["age"].roll(1, 0)}, "do(brain_volume)": {"brain_volume": pa["brain_volume"] * 0.5},
           "null": {}}
    rng = _rng_state(m)
    imgs = ev.effectiveness(dict(pa, x=x), dos, return_images=True)
    res = ev.results()["effectiveness"]
    _check_effectiveness(ev, pred, scm, pa, dos, imgs, res, cf_eval.metric_specs("ukbb", raw=False))
    # age came through the host-side MLP: its raw output is that MLP's loc on the counterfactual volumes, not a CNN head
    cf_pa = scm.counterfactual(obs=pa, intervention=dos["do(age)"], num_particles=1)
    raw = pred.raw_outputs(x=imgs["do(age)"], **cf_pa)
    ctx = torch.cat([cf_pa["brain_volume"], cf_pa["ventricle_volume"]], -1)
    assert torch.equal(raw["age"], pred.encoder_a(ctx)[:, :1]) and raw["sex"].stride(0) == 16
    want = _replayed_images(m, ev, x, pa, scm, dos, rng)
    for k in dos:
        assert torch.equal(imgs[k], want[k]), k


def test_predictor_eval_on_three_batches(morpho):
    from causal_gen_amd import cf_eval

    hp, m, scm, pred, _, _ = morpho
    g = torch.Generator().manual_seed(31)
    batches = []
    for B in (4, 3, 5):
        pa = scm.sample(B, g)
        batches.append(dict(pa, x=((torch.randint(0, 256, (B, 1, 32, 32), generator=g).float() - 127.5) / 127.5).cuda()))
    specs = cf_eval.metric_specs("morphomnist")
    got = cf_eval.predictor_eval(pred, batches, specs)
    preds = [pred.predict(**b) for b in batches]
    for s in cf_eval.metric_specs("morphomnist", raw=False):
        p = torch.cat([q[s.name] for q in preds]).detach().cpu().numpy()
        t = torch.cat([b[s.name] for b in batches]).detach().cpu().numpy()
        want = R.spec_metrics(s, p, t)
        assert got["n"][s.name] == want["n"] == 12
        for mname in s.metrics:
            key = s.name + "_" + mname
            tol = 1e-6 * abs(want[key]) if mname == "mae" else 0.0
            assert abs(got[key] - want[key]) <= tol, (key, got[key], want[key])
    # the same through the {"x", "pa"} batches of a DeviceLoader with a column map
    packed = [{"x": b["x"], "pa": torch.cat([b["thickness"], b["intensity"], b["digit"]], 1)} for b in batches]
    got2 = cf_eval.predictor_eval(pred, packed, specs, columns={"thickness": 0, "intensity": 1, "digit": (2, 10)})
    assert repr(got2) == repr(got)
