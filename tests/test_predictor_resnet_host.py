"""ChestPredictor without a GPU: the reference's 248 state-dict keys on one shared trunk, loading a reference checkpoint,
deepcopy, the plain-torch restatement against the tests' f64 oracle, shape checks, and the metric table for raw heads."""
import copy
from types import SimpleNamespace

import pytest
import torch

from resnet_ref import VARS, chest_ref, make_obs, randomise


def _args(res=64, **kw):
    return SimpleNamespace(input_channels=1, input_res=res, std_fixed=0.0, dataset="mimic224", **kw)


def _pred(res=64, seed=0):
    from causal_gen_amd.predictor_resnet import ChestPredictor

    return randomise(ChestPredictor(_args(res)), seed)


def test_state_dict_has_exactly_the_reference_keys():
    import causal_gen_amd
    from causal_gen_amd.predictor_resnet import ChestPredictor

    assert causal_gen_amd.ChestPredictor is ChestPredictor
    pred = _pred()
    sd = pred.state_dict()
    assert len(sd) == 248
    for enc in ("encoder_s", "encoder_r", "encoder_f", "encoder_a"):
        keys = [k for k in sd if k.startswith(enc + ".")]
        assert len(keys) == 62, enc
        assert len([k for k in keys if ".resnet." in k]) == 60
        for k in ("resnet.0.weight", "resnet.1.weight", "resnet.1.bias", "resnet.4.0.conv1.weight", "resnet.4.1.bn2.bias",
                  "resnet.5.0.downsample.0.weight", "resnet.5.0.downsample.1.weight", "resnet.6.0.downsample.1.bias",
                  "resnet.7.0.downsample.0.weight", "resnet.7.1.conv2.weight", "resnet.7.1.bn1.weight", "fc.weight", "fc.bias"):
            assert f"{enc}.{k}" in sd, (enc, k)
        assert f"{enc}.resnet.4.0.downsample.0.weight" not in sd and f"{enc}.resnet.5.1.downsample.0.weight" not in sd
    assert not list(pred.buffers())
    assert tuple(sd["encoder_s.resnet.0.weight"].shape) == (64, 1, 7, 7)
    assert tuple(sd["encoder_s.resnet.6.0.downsample.0.weight"].shape) == (256, 128, 1, 1)
    assert [tuple(sd[f"encoder_{e}.fc.weight"].shape) for e in "srfa"] == [(1, 512), (3, 512), (1, 512), (2, 513)]
    groups = {m.num_channels: m.num_groups for m in pred.modules() if isinstance(m, torch.nn.GroupNorm)}
    assert groups == {64: 16, 128: 32, 256: 32, 512: 32}


def test_the_four_heads_share_one_trunk():
    pred = _pred()
    assert pred.encoder_r.resnet is pred.encoder_s.resnet is pred.encoder_f.resnet is pred.encoder_a.resnet
    sd = pred.state_dict()
    for k in [k for k in sd if k.startswith("encoder_s.resnet.")]:
        for enc in ("encoder_r", "encoder_f", "encoder_a"):
            assert sd[k].data_ptr() == sd[k.replace("encoder_s", enc)].data_ptr(), k
    assert len(list(pred.parameters())) == 60 + 8
    assert pred.training is False and pred.train().training is False
    dup = copy.deepcopy(pred)
    assert dup.encoder_a.resnet is dup.encoder_s.resnet and dup.encoder_s.resnet is not pred.encoder_s.resnet
    assert all(torch.equal(a, b) for a, b in zip(dup.state_dict().values(), sd.values()))
    assert not any(k in dup.__dict__ for k in ("_ws", "_rt", "_ws_token", "_ws_shape"))


def test_load_reference_state_dict_round_trips_and_returns_the_extras():
    from causal_gen_amd import predictor as P
    from causal_gen_amd.predictor_resnet import ChestPredictor

    src = _pred(seed=3)
    sd = {k: v.clone() for k, v in src.state_dict().items()}  # four separate, equal trunk copies: a reference checkpoint
    extra = {"sex_logit": torch.zeros(1), "race_logits": torch.zeros(1, 3), "age_flow_components.unnormalized_widths": torch.zeros(1, 4),
             "finding_transform_GumbelMax.context_nn.layers.0.weight": torch.zeros(8, 1)}
    dst = ChestPredictor(_args())
    assert dst.load_reference_state_dict(dict(sd, **extra)) == sorted(extra)
    for k, v in dst.state_dict().items():
        assert torch.equal(v, sd[k]), k
    with pytest.raises(RuntimeError):
        dst.load_reference_state_dict({k: v for k, v in sd.items() if k != "encoder_a.fc.bias"})
    bad = dict(sd)
    bad["encoder_r.resnet.0.weight"] = sd["encoder_r.resnet.0.weight"] + 1
    with pytest.raises(ValueError, match="share one trunk"):
        dst.load_reference_state_dict(bad)
    with pytest.raises(NotImplementedError, match="ResNet"):
        P.make_predictor(_args(224))


@pytest.mark.parametrize("R,B", [(33, 3), (64, 2)])
def test_torch_outputs_in_f64_equals_the_oracle(R, B):
    pred = _pred(R, seed=5)
    obs = make_obs(B, R, seed=6)
    ref = chest_ref(pred.state_dict(), obs)
    for shared in (True, False):
        got = pred.torch_outputs(obs["x"].double(), obs["finding"].double(), shared=shared)
        for var in VARS:
            assert got[var].dtype == torch.float64 and got[var].shape == ref["outs"][var].shape
            assert (got[var] - ref["outs"][var]).abs().max() <= 1e-12 * max(1.0, ref["outs"][var].abs().max().item()), var
    f32 = pred.torch_outputs(obs["x"], obs["finding"])
    assert all(f32[v].dtype == torch.float32 and (f32[v].double() - ref["outs"][v]).abs().max() < 1e-4 for v in VARS)
    maps = [a.shape[-1] for a in ref["acts"]]
    h1 = (R - 1) // 2 + 1
    assert len(maps) == 18 and maps[0] == h1 and maps[17] == maps[1] == (h1 - 1) // 2 + 1 and len(ref["pres"]) == 17


def test_unsupported_shapes_raise_before_device_work():
    from causal_gen_amd.predictor_resnet import ChestPredictor

    pred = ChestPredictor(_args(64))
    for x in (torch.zeros(2, 1, 32, 32), torch.zeros(2, 1, 64, 48), torch.zeros(2, 3, 64, 64), torch.zeros(0, 1, 64, 64), torch.zeros(1, 64, 64)):
        with pytest.raises(ValueError, match="ChestPredictor"):
            pred._check(x)
    for res in (16, 31, 257, 512):
        with pytest.raises(ValueError, match="32..256"):
            ChestPredictor(_args(res))._check(torch.zeros(1, 1, res, res))
    with pytest.raises(ValueError, match="input_channels"):
        ChestPredictor(SimpleNamespace(input_channels=3, input_res=64, std_fixed=0.0))._check(torch.zeros(1, 3, 64, 64))
    assert pred.path(torch.zeros(1, 1, 64, 64)) == "resnet"
    with pytest.raises(NotImplementedError, match="training"):  # (what PredictorTrainStep would ask for: no silent empty step)
        pred._heads()
    assert ChestPredictor(_args(64, )).std_fixed == 0.0 and ChestPredictor(SimpleNamespace(input_channels=1, input_res=64, std_fixed=0.3)).std_fixed == 0.3


def test_chest_metric_specs_is_the_mimic_table_with_the_raw_transforms():
    from dataclasses import replace

    from causal_gen_amd import cf_eval

    base = cf_eval.metric_specs("mimic")
    raw = cf_eval.chest_metric_specs()
    assert [s.name for s in raw] == [s.name for s in base]
    assert {s.name: s.transform for s in raw} == {"sex": "sigmoid", "finding": "sigmoid", "race": "softmax", "age": "none"}
    assert [replace(s, transform="none") for s in raw] == base
    assert cf_eval.chest_metric_specs(raw=False) == base
    age = next(s for s in raw if s.name == "age")
    assert (age.pred_scale, age.pred_shift, age.tgt_scale, age.tgt_shift) == (50.0, 50.0, 50.0, 50.0)
