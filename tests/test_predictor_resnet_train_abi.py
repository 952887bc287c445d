"""ChestPredictorTrainStep's entry points without a GPU: exported, declared and bound at ABI 411, bad arguments
rejected before any launch with a message that names them, the eval workspace not grown; and the f64 helper of the GPU tests
(tests/resnet_train_ref.py) held together on the CPU.  (The record's layout against the header: tests/test_abi_mirror.py.)"""
import ctypes as C
import os
import re
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from conftest import ROOT

NAMES = ("cgen_resnet_train_workspace", "cgen_resnet_train_fwd", "cgen_resnet_train_bwd", "cgen_resnet_dropout_keep")
FAKE = 4096  # a fake device address: validation must reject before anything dereferences it
# cgen_resnet_workspace(n, res) as the commit before the training entry points returned it
EVAL_WS = {(1, 32): 166632, (3, 33): 673824, (2, 64): 1325904, (2, 96): 2980304, (2, 192): 11914064, (32, 192): 190625024,
           (32, 224): 259448064, (4, 256): 42357408}


def _args(**kw):
    from causal_gen_amd import _lib

    a = _lib.ResnetTrainArgs()
    a.net.res, a.net.ctx, a.net.ctx_stride = 64, FAKE, 1
    for i in range(_lib.RESNET_CONVS):
        a.net.img_fwd[i] = a.net.img_dg[i] = a.net.gamma[i] = a.net.beta[i] = FAKE
        a.gw[i] = a.ggamma[i] = a.gbeta[i] = FAKE
    for h in range(4):
        a.net.fc_w[h] = a.net.fc_b[h] = a.net.obs[h] = a.gfc_w[h] = a.gfc_b[h] = FAKE
        a.net.obs_stride[h] = 3 if h == 1 else 1
    a.rng, a.p_dropout = FAKE, 0.2
    for k, v in kw.items():
        if k == "res":
            a.net.res = v
        else:
            setattr(a, k, v)
    return a


def test_train_symbols_are_exported_declared_and_bound_at_abi_411():
    from causal_gen_amd import _lib

    header = open(os.path.join(ROOT, "include", "cgen_hip.h")).read()
    assert re.search(r"#define CGEN_ABI_VERSION 411\b", header)
    lib = _lib.load()
    assert lib.version() == 411 == _lib.ABI_VERSION
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(lib.cdll, name), name
    import causal_gen_amd

    assert causal_gen_amd.ChestPredictorTrainStep.__name__ == "ChestPredictorTrainStep"


def test_train_entry_points_reject_bad_arguments_before_any_launch():
    from causal_gen_amd import _lib

    lib = _lib.load()
    need = _lib.i64(0)
    lib.resnet_train_workspace(2, 64, C.byref(need))
    big = need.value

    def fwd(a, n=2, x=FAKE, ws=FAKE, ws_floats=None, terms=FAKE, outs=None, loss=None):
        return lib._raw_cgen_resnet_train_fwd(C.byref(a) if a is not None else None, n, x, ws, big if ws_floats is None else ws_floats,
                                              terms, outs, loss, None)

    def bwd(a, n=2, x=FAKE, ws=FAKE, ws_floats=None, coef=FAKE, dx=FAKE):
        return lib._raw_cgen_resnet_train_bwd(C.byref(a) if a is not None else None, n, x, ws, big if ws_floats is None else ws_floats,
                                              coef, dx, None)

    def keep(rng=FAKE, p=0.2, n=2, res=64, k=0, out=FAKE):
        return lib._raw_cgen_resnet_dropout_keep(rng, p, n, res, k, out, None)

    eval_need = _lib.i64(0)
    lib.resnet_workspace(2, 64, C.byref(eval_need))
    no_img, no_gamma, no_fc, no_obs, no_gw, odd_gw, odd_gg, no_gb, no_gfc, odd_gfc = (_args() for _ in range(10))
    no_img.net.img_fwd[7] = None
    no_gamma.net.gamma[3] = None
    no_fc.net.fc_w[2] = None
    no_obs.net.obs[1] = None
    no_gw.gw[5] = None
    odd_gw.gw[6] = FAKE + 4
    odd_gg.ggamma[2] = FAKE + 8
    no_gb.gbeta[19] = None
    no_gfc.gfc_b[3] = None
    odd_gfc.gfc_w[1] = FAKE + 2
    for run, who in ((fwd, "cgen_resnet_train_fwd"), (bwd, "cgen_resnet_train_bwd")):
        cases = [
            (lambda: run(None), "null args"),
            (lambda: run(_args(), n=0), "n = 0"),
            (lambda: run(_args(), n=-3), "n = -3"),
            (lambda: run(_args(res=31)), "res = 31"),
            (lambda: run(_args(res=257)), "res = 257"),
            (lambda: run(_args(), x=None), "null x"),
            (lambda: run(_args(), ws=None), "ws is null"),
            (lambda: run(_args(), ws=FAKE + 4), "16-byte aligned"),
            (lambda: run(_args(), ws_floats=big - 1), "ws_floats"),
            (lambda: run(_args(), ws_floats=eval_need.value), "ws_floats"),  # (the eval workspace is too small)
            (lambda: run(_args(p_dropout=1.0)), "p_dropout = 1"),
            (lambda: run(_args(p_dropout=-0.1)), "p_dropout = -0.1"),
            (lambda: run(_args(p_dropout=float("nan"))), "p_dropout"),
            (lambda: run(_args(rng=None)), "null rng"),
            (lambda: run(no_img), "weight image 7"),
            (lambda: run(no_gamma), "gamma / beta 3"),
            (lambda: run(no_fc), "fc_w / fc_b of head 2"),
            (lambda: run(no_obs), "obs of head 1"),
        ]
        for call, words in cases:
            assert call() < 0, (who, words)
            msg = lib.last_error().decode()
            assert words in msg and who in msg, (words, msg)
    for call, words in [
        (lambda: fwd(_args(), terms=None), "null terms"),
        (lambda: bwd(_args(), coef=None), "null coef_dev"),
        (lambda: bwd(no_gw), "gw 5"),
        (lambda: bwd(odd_gw), "gw 6"),
        (lambda: bwd(odd_gg), "ggamma / gbeta 2"),
        (lambda: bwd(no_gb), "ggamma / gbeta 19"),
        (lambda: bwd(no_gfc), "gfc_w / gfc_b of head 3"),
        (lambda: bwd(odd_gfc), "gfc_w / gfc_b of head 1"),
        (lambda: keep(rng=None), "null rng"),
        (lambda: keep(out=None), "keep is null"),
        (lambda: keep(p=1.0), "p_dropout = 1"),
        (lambda: keep(n=0), "n = 0"),
        (lambda: keep(res=300), "res = 300"),
        (lambda: keep(k=8), "block = 8"),
        (lambda: keep(k=-1), "block = -1"),
    ]:
        assert call() < 0, words
        msg = lib.last_error().decode()
        assert words in msg and "cgen_resnet_" in msg, (words, msg)
    assert lib._raw_cgen_resnet_train_workspace(2, 64, None) < 0 and "null floats" in lib.last_error().decode()
    assert lib._raw_cgen_resnet_train_workspace(0, 64, C.byref(need)) < 0 and "n = 0" in lib.last_error().decode()
    assert lib._raw_cgen_resnet_train_workspace(2, 24, C.byref(need)) < 0 and "res = 24" in lib.last_error().decode()


def test_the_eval_workspace_has_not_grown_and_the_training_one_holds_it():
    from causal_gen_amd import _lib

    lib = _lib.load()
    for (n, res), want in EVAL_WS.items():
        ev, tr = _lib.i64(0), _lib.i64(0)
        lib.resnet_workspace(n, res, C.byref(ev))
        lib.resnet_train_workspace(n, res, C.byref(tr))
        assert ev.value == want, (n, res)
        assert tr.value > ev.value and tr.value % 4 == 0, (n, res)


def test_the_f64_helper_pinned_with_its_own_masks_is_the_free_run():
    import resnet_train_ref as T
    from resnet_ref import make_obs, randomise

    from causal_gen_amd.predictor_resnet import ChestPredictor

    R, B = 33, 3
    pred = randomise(ChestPredictor(SimpleNamespace(input_channels=1, input_res=R, std_fixed=0.0)), 100)
    obs = make_obs(B, R, 200)
    sd = {k: v.detach() for k, v in pred.state_dict().items()}
    names = T.param_names(sd)
    assert names == [n for n, _ in pred.named_parameters()] and len(names) == 68
    free = T.loss_and_grads_ref(sd, obs)
    masks = [(p > 0).double() for p in free["pres"]]
    pool_idx = F.max_pool2d(free["acts"][0], 3, 2, 1, return_indices=True)[1]
    pinned = T.loss_and_grads_ref(sd, obs, masks=masks, pool_idx=pool_idx)
    rel = lambda a, b: float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)
    assert rel(pinned["loss"], free["loss"]) <= 1e-12 and rel(pinned["x"], free["x"]) <= 1e-12
    assert set(free["grads"]) == set(names)
    for n in names:
        assert free["grads"][n].shape == sd[n].shape and float(free["grads"][n].abs().max()) > 0, n
        assert rel(pinned["grads"][n], free["grads"][n]) <= 1e-12, n
    # Dropout through the masks: keep everything at p = 0 is the free run; a real mask scales what it keeps and moves the loss
    keeps = [torch.ones_like(masks[s], dtype=torch.bool) for s in T.A1_SITES]
    same = T.loss_and_grads_ref(sd, obs, masks=T.dropout_masks(masks, keeps, 0.0), pool_idx=pool_idx)
    assert rel(same["loss"], free["loss"]) <= 1e-12
    g = torch.Generator().manual_seed(0)
    keeps = [torch.rand(masks[s].shape, generator=g) >= 0.2 for s in T.A1_SITES]
    drop = T.loss_and_grads_ref(sd, obs, masks=T.dropout_masks(masks, keeps, 0.2), pool_idx=pool_idx)
    a1 = drop["acts"][T.A1_SITES[0]]
    assert bool((a1[~keeps[0]] == 0).all()) and rel(a1[keeps[0]], (free["acts"][T.A1_SITES[0]] / 0.8)[keeps[0]]) <= 1e-12
    assert abs(float(drop["loss"]) - float(free["loss"])) > 1e-6
    # the f64 loop learns the (32, 4) batch of the GPU test at lr = 1e-3
    pred = randomise(ChestPredictor(SimpleNamespace(input_channels=1, input_res=32, std_fixed=0.0)), 100)
    losses = T.f64_loop({k: v.detach() for k, v in pred.state_dict().items()}, make_obs(4, 32, 200), 20, 1e-3)
    print(f"f64 loop on (32, 4): {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert losses[-1] < losses[0] - 0.1
