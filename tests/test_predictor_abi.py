"""Anticausal predictors without a GPU: argument validation before any launch, a clean gfx950 code object, and the module
surface (reference state-dict names, the f64 oracle against the reference CNN's own outputs)."""
import re
from types import SimpleNamespace

import pytest
import torch

import codeobj
from conftest import load_golden
from predictor_ref import cnn_ref


def _rec(**kw):
    from causal_gen_amd import _lib

    r = _lib.PredHead()
    r.c, r.res, r.width, r.nout, r.ctx, r.kind, r.obs_stride = 1, 32, 8, 2, 0, _lib.PRED_NORMAL, 1
    for i in range(8):
        r.w[i], r.b[i] = 4096, 4096  # fake device addresses: validation must reject before anything dereferences them
    r.obs = 4096
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _fwd(lib, rec, n=2):
    from causal_gen_amd import _lib

    recs = (_lib.PredHead * 1)(rec)
    return lib._raw_cgen_predictor_fwd(recs, 1, n, 8192, None, 12288, None, None, None)


def test_predictor_entry_points_reject_bad_records():
    from causal_gen_amd import _lib

    lib = _lib.load()
    bad_w = _rec()
    bad_w.w[3] = None
    cases = [
        (_rec(kind=7), "unknown variable kind"),
        (bad_w, "null weight pointer"),
        (_rec(ctx=1), "context mismatch"),
        (_rec(y=4096), "context mismatch"),
        (_rec(width=12), "unsupported width"),
        (_rec(nout=3), "do not fit variable kind"),
        (_rec(res=4), "unsupported input shape"),
    ]
    for rec, words in cases:
        assert _fwd(lib, rec) < 0, words
        msg = lib.last_error().decode()
        assert words in msg, (words, msg)
    # the fused (LDS) entry does not take a 192x192 image; the check runs before the launch
    big = (_lib.PredHead * 1)(_rec(res=192, width=16))
    assert lib._raw_cgen_predictor_supported(big, 1) == 0
    assert lib._raw_cgen_predictor_fwd(big, 1, 2, 8192, None, 12288, None, None, None) < 0
    assert "fused path does not take" in lib.last_error().decode()
    small = (_lib.PredHead * 1)(_rec())
    assert lib._raw_cgen_predictor_supported(small, 1) == 1
    with pytest.raises(_lib.CgenError, match="cgen_predictor_bwd"):
        lib.predictor_bwd(small, 1, 2, 8192, None, None, 12288, None)


def test_predictor_kernels_have_no_scratch_and_no_spills():
    seen = set()
    for name, scratch, spills in codeobj.kernels():
        k = re.search(r"(predictor_kernelILb[01]ELb[01]E|pred_sum_kernel)", name)
        if not k:
            continue
        seen.add(k.group(1))
        assert scratch == 0, (name, scratch)
        assert spills == 0, (name, spills)
    assert len(seen) == 5, sorted(seen)


@pytest.mark.parametrize("tag", ["morphomnist", "cmnist"] + [f"ukbb192_encoder_{h}" for h in "vbsm"])
def test_cnn_loads_reference_state_dicts_and_oracle_matches_reference(tag):
    from causal_gen_amd.predictor import CNN

    gd = load_golden(f"predictor_{tag}.pt")
    x = gd["x"].double().requires_grad_(True)
    for name, h in gd["heads"].items():
        cnn = CNN(gd["in_shape"], width=h["width"], num_outputs=h["nout"], context_dim=h["ctx"])
        cnn.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in h["state_dict"].items()}, strict=True)
        y = h["y"].double() if h["y"] is not None else None
        out = cnn_ref(cnn, x, y)
        assert torch.allclose(out.detach(), h["out64"], rtol=0, atol=1e-10 * h["out64"].abs().max().item()), name
        (gx,) = torch.autograd.grad((out * h["wout"].double()).sum(), x)
        assert (gx.float() - h["gx64"]).abs().max() <= 1e-6 * h["gx64"].abs().max(), name


def test_load_reference_state_dict_keeps_exactly_the_encoders():
    from causal_gen_amd import predictor as P

    args = SimpleNamespace(input_channels=1, input_res=32, std_fixed=0.0, dataset="morphomnist")
    src = P.make_predictor(args)
    sd = dict(src.state_dict())
    extra = {"digit_logits": torch.zeros(1, 10), "t_base_loc": torch.zeros(1), "thickness_module.0.unnormalized_widths": torch.zeros(1, 4),
             "context_nn.nn.layers.0.weight": torch.zeros(4, 1)}
    full = dict(sd, **extra)
    dst = P.MorphoMNISTPredictor(args)
    dropped = dst.load_reference_state_dict(full)
    assert dropped == sorted(extra)
    for k, v in dst.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert sorted(k.split(".")[0] for k in sd if k.endswith("cnn.0.weight")) == ["encoder_i", "encoder_t", "encoder_y"]
    with pytest.raises(NotImplementedError, match="ResNet"):
        P.make_predictor(SimpleNamespace(dataset="mimic", input_channels=1, input_res=224, std_fixed=0.0))
    ukbb = P.FlowPredictor(SimpleNamespace(input_channels=1, input_res=192, std_fixed=0.0))
    assert {k.split(".")[0] for k in ukbb.state_dict()} == {"encoder_s", "encoder_m", "encoder_a", "encoder_b", "encoder_v"}
    assert "encoder_a.mlp.6.bias" in ukbb.state_dict() and "encoder_v.fc.3.weight" in ukbb.state_dict()
