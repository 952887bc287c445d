"""The predictors' device-side input on the MI355X: the planar arm of the input pipeline (``DeviceDataset.batch(planar=True)``,
cgen_batch_augment_planar) against the NHWC launch bit for bit, and ``PredictorTrainStep.step_from`` -- the batch built inside
the captured step from a data set whose ``pa`` holds every variable -- against a twin that is handed the same batch through
``step()``, bit for bit in every parameter, buffer and moment."""
from types import SimpleNamespace

import pytest
import torch

from predictor_ref import randomise

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ds(n_data, c, h0, w0, res, pad, hflip, ctx=3, seed=0):
    from causal_gen_amd.data import DeviceDataset

    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (n_data, c, h0, w0), generator=g, dtype=torch.uint8)
    pa = torch.rand(n_data, ctx, generator=g)
    return DeviceDataset(x, pa, res, pad=pad, hflip=hflip)


# (c, h0, w0, crop, (pad_x, pad_y), hflip, index)
PLANAR = {
    "c3_28_to_32_flips": (3, 28, 28, 32, (4, 4), 0.5, [3, 0, 99, 7, 3]),  # row 99 of 10 is out of range: padding value, draws -1
    "c2_9x7_to_5x6": (2, 9, 7, (5, 6), (1, 0), 0.5, [1, 2, 3]),
    "c4_8_to_8": (4, 8, 8, 8, (0, 0), 0.0, [9, 8]),
}


@pytest.mark.parametrize("tag", sorted(PLANAR))
def test_planar_batch_equals_the_nhwc_batch(tag):
    c, h0, w0, res, pad, hflip, idx = PLANAR[tag]
    ds = _ds(10, c, h0, w0, res, pad, hflip)
    index = torch.tensor(idx, device="cuda")
    n = len(idx)
    my, mx = ds.draw_range()
    g = torch.Generator().manual_seed(1)
    draws = torch.stack([torch.randint(0, my + 1, (n,), generator=g), torch.randint(0, mx + 1, (n,), generator=g),
                         torch.randint(0, 2 if hflip else 1, (n,), generator=g)], dim=1).int()
    a = ds.batch(index, draws=draws, planar=True)
    b = ds.batch(index, draws=draws)
    assert a["x"].is_contiguous() and tuple(a["x"].shape) == (n, c, ds.r_h, ds.r_w) and a["x"].dtype == torch.float32
    assert not b["x"].is_contiguous() or c == 1
    assert torch.equal(_bits(a["x"]), _bits(b["x"].contiguous()))
    assert torch.equal(_bits(a["pa"]), _bits(b["pa"]))
    valid = [0 <= r < 10 for r in idx]
    want = (ds.reference_batch(index, draws).float() - 127.5) * (1 / 127.5)  # (the u8 batch the reference's transforms give)
    got = a["x"].cpu()
    for i, ok in enumerate(valid):
        if ok:
            assert (got[i] - want[i]).abs().max() <= 1e-6, i
        else:
            assert float((got[i] + 1.0).abs().max()) <= 1e-6 and bool((a["pa"][i] == 0).all())  # padding value 0 -> -1


def test_planar_batch_draws_what_the_nhwc_batch_draws():
    c, h0, w0, res, pad, hflip, idx = PLANAR["c3_28_to_32_flips"]
    ds = _ds(10, c, h0, w0, res, pad, hflip)
    index = torch.tensor(idx, device="cuda")
    rng = torch.tensor([1234, 5], dtype=torch.int64, device="cuda")
    a = ds.batch(index, rng=rng, return_draws=True, planar=True)
    b = ds.batch(index, rng=rng, return_draws=True)
    assert torch.equal(a["draws"], b["draws"]) and a["draws"][2].tolist() == [-1, -1, -1]
    assert len({tuple(r) for r in a["draws"].tolist()}) > 2  # (real draws, not a constant)
    assert torch.equal(a["draws"][0], a["draws"][4])  # the repeated row draws the same crop: keyed by the data set row
    assert torch.equal(_bits(a["x"]), _bits(b["x"].contiguous()))
    from causal_gen_amd import _lib

    with pytest.raises(ValueError, match="planar batch is f32"):
        ds.batch(index, rng=rng, planar=True, dtype=torch.bfloat16 if _lib.load().h16_is_bf16 else torch.float16)


# ------------------------------------------------------------------------------------------------ step_from
UKBB_COLS = {"sex": 0, "mri_seq": 1, "age": 2, "brain_volume": 3, "ventricle_volume": 4}
CMNIST_COLS = {"digit": (0, 10), "colour": (10, 10)}


def _ukbb():
    """(predictor, data set: 16 rows of 1 x 10 x 10 cropped to 9 x 9 with flips, pa = every variable, columns)"""
    from causal_gen_amd import predictor as Pm
    from causal_gen_amd.data import DeviceDataset

    g = torch.Generator().manual_seed(0)
    pred = Pm.make_predictor(SimpleNamespace(dataset="ukbb192", input_channels=1, input_res=9, std_fixed=0.0))
    randomise(pred, g)
    x = torch.randint(0, 256, (16, 1, 10, 10), generator=g, dtype=torch.uint8)
    pa = torch.rand(16, 5, generator=g) * 1.6 - 0.8
    pa[:, :2] = torch.randint(0, 2, (16, 2), generator=g).float()
    return pred, DeviceDataset(x, pa, 9, pad=(0, 0), hflip=0.5), UKBB_COLS


def _cmnist():
    from causal_gen_amd import predictor as Pm
    from causal_gen_amd.data import DeviceDataset

    g = torch.Generator().manual_seed(0)
    pred = Pm.make_predictor(SimpleNamespace(dataset="cmnist", input_channels=3, input_res=32, std_fixed=0.0))
    randomise(pred, g)
    x = torch.randint(0, 256, (16, 3, 28, 28), generator=g, dtype=torch.uint8)
    oh = lambda: torch.nn.functional.one_hot(torch.randint(0, 10, (16,), generator=g), 10).float()
    return pred, DeviceDataset(x, torch.cat([oh(), oh()], dim=1), 32, pad=(4, 4), hflip=0.0), CMNIST_COLS


def _state(ts, pred):
    out = dict(p=ts._on.flat_p, b=ts._on.flat_b, ep=ts._ema.flat_p, eb=ts._ema.flat_b, m=ts.m, v=ts.v, state=ts.state)
    for k, v in pred.state_dict().items():
        out["sd." + k] = v.float()
    for k, v in ts.ema_model.state_dict().items():
        out["esd." + k] = v.float()
    return out


@pytest.mark.parametrize("graph", (True, False), ids=("captured", "eager"))
@pytest.mark.parametrize("make", (_ukbb, _cmnist), ids=("ukbb", "cmnist"))
def test_step_from_equals_step_on_the_same_batch(make, graph):
    from causal_gen_amd.predictor_train import PredictorTrainStep

    kw = dict(lr=1e-3, ema_update_after=0, use_graph=graph, scalar_heads=True)
    pred, ds, cols = make()
    twin_pred, _, _ = make()
    ts = PredictorTrainStep(pred, columns=cols, **kw)
    twin = PredictorTrainStep(twin_pred, **kw)
    for k, v in _state(ts, pred).items():
        assert torch.equal(_bits(v), _bits(_state(twin, twin_pred)[k])), k
    B = 5
    d = torch.full((B, 3), -7, dtype=torch.int32, device="cuda")
    seen = []
    for i, idx in enumerate(([3, 11, 3, 0, 15], [1, 2, 2, 14, 9], [8, 8, 4, 5, 6])):  # (each with a repeated row)
        index = torch.tensor(idx, device="cuda")
        out = ts.step_from(ds, index, draws_out=d)
        torch.cuda.synchronize()
        assert len(ts._graphs) == (1 if graph else 0)  # another index replays the same graph
        seen.append(d.clone())
        my, mx = ds.draw_range()
        assert bool(((d[:, 0] >= 0) & (d[:, 0] <= my) & (d[:, 1] >= 0) & (d[:, 1] <= mx) & (d[:, 2] >= 0) & (d[:, 2] <= 1)).all())
        rows = ds.pa[index]
        obs = {var: rows[:, c:c + 1] if isinstance(c, int) else rows[:, c[0]:c[0] + c[1]] for var, c in cols.items()}
        want = twin.step(x=ds.batch(index, draws=d)["x"], **obs)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out["loss"]), _bits(want["loss"])) and torch.equal(_bits(out["grad_norm"]), _bits(want["grad_norm"])), i
        got, ref = _state(ts, pred), _state(twin, twin_pred)
        assert set(got) == set(ref)
        for k in got:
            assert torch.equal(_bits(got[k]), _bits(ref[k])), (i, k)
    assert ts.it == 3 and ts.stats()["opt_steps"] == 3
    if ds.draw_range() != (0, 0):
        assert not all(torch.equal(seen[0], s) for s in seen[1:])  # fresh draws on every replay
    assert int(ts._rng[1]) == 3  # the class's own Philox state moved on once per step


def test_step_from_rejects_missing_columns_before_any_device_work():
    from causal_gen_amd.predictor_train import PredictorTrainStep

    pred, ds, cols = _ukbb()
    index = torch.tensor([0, 1, 2, 3], device="cuda")
    ts = PredictorTrainStep(pred, scalar_heads=True)
    with pytest.raises(ValueError, match="name the columns"):
        ts.step_from(ds, index)
    ts = PredictorTrainStep(_ukbb()[0], scalar_heads=True, columns={k: v for k, v in cols.items() if k != "age"})
    with pytest.raises(ValueError, match="no column was named for \\['age'\\]"):
        ts.step_from(ds, index)
    assert not ts._statics and not ts._graphs and ts.it == 0 and ts._rng is None
    # without the scalar head "age" is not needed
    ts = PredictorTrainStep(_ukbb()[0], columns={k: v for k, v in cols.items() if k != "age"})
    out = ts.step_from(ds, index)
    assert bool(torch.isfinite(out["loss"]))
    ts = PredictorTrainStep(_ukbb()[0], scalar_heads=True, columns=dict(cols, age=5))
    with pytest.raises(ValueError, match="do not fit"):
        ts.step_from(ds, index)


def test_an_epoch_through_step_from_lowers_the_age_term():
    """A UKBB predictor trained only through step_from: finite losses and a decreasing age term"""
    from causal_gen_amd.data import DeviceLoader
    from causal_gen_amd.predictor_train import PredictorTrainStep

    pred, ds, cols = _ukbb()
    ts = PredictorTrainStep(pred, lr=1e-2, scalar_heads=True, columns=cols)
    loader = DeviceLoader(ds, 8, shuffle=False)
    age = []
    for _ in range(12):
        for idx in loader.indices():
            assert bool(torch.isfinite(ts.step_from(ds, idx)["loss"]))
            (ent,) = ts._statics.values()
            age.append(float(ent["scalars"][0][2].mean()))
    first, last = sum(age[:4]) / 4, sum(age[-4:]) / 4
    print(f"age term {first:.4f} -> {last:.4f} over {len(age)} steps")
    assert last < first
