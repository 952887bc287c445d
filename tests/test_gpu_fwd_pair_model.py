"""The forward pair launch in the model (CGEN_BLK3_FWD_PAIR): a small HVAE with layers at 24 x 24, 12 x 12, 6 x 6 and 1 x 1, batch 3.
Knob on against knob off: ELBO, NLL, KL, the collected z and every parameter gradient bit for bit; one forward launch fewer per
served layer, the backward launches unchanged; the counter; a non-recording abduction pass; three graph-replayed train steps.

"narrow" is the small model of the latent-tail tests (widths 32 .. 128: bottlenecks 24 at 6 x 6 and 16 at 12 x 12 pair on the small-
image instance; the 24 x 24 layers have a bottleneck of 8, whose tile pair is not compiled, and keep the fork).  "wide" puts the
widths of ukbb192 at those sizes (128 / 160 / 192): the 24 x 24 layers pair on the tile instance <4, 1, 8, 4, 8> as well."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

WIDTHS = {"narrow": ([32, 64, 96, 128], 4), "wide": ([128, 160, 192, 256], 6)}  # widths, served layers (two per served size)


def _hp(kind, **over):
    from causal_gen_amd.hps import setup_hparams

    return setup_hparams("ukbb192", input_res=24, enc_arch="24b1d2,12b1d2,6b1d6,1b1", dec_arch="1b1,6b2,12b2,24b2",
                         widths=WIDTHS[kind][0], z_max_res=24, z_dim=16, bs=3, **over)


def _model(hp):
    from causal_gen_amd import vae

    torch.manual_seed(7)
    m = vae.HVAE(hp)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for p in m.parameters():  # (the reference zero-initialises the prior heads: every conv gets weight, scaled to its fan-in)
            p.add_(torch.randn(p.shape, generator=g) * (0.05 if p.dim() < 4 else 0.5 / p[0].numel() ** 0.5))
    m.compute_dtype = "f16"
    return m.cuda().train()


def _batch(hp, B=3):
    g = torch.Generator().manual_seed(1)
    R = hp.input_res
    x = (torch.randint(0, 256, (B, 1, R, R), generator=g).float() - 127.5) / 127.5
    pa = torch.randn(B, hp.context_dim, generator=g)
    return x.cuda(), pa.cuda()[..., None, None].expand(-1, -1, R, R)


def _seed(eng):
    eng.rng_ptr()
    eng.rng.copy_(torch.tensor([11, 0], dtype=torch.int64, device=eng.rng.device))


def _one_pass(monkeypatch, knob, kind, serial="1"):
    monkeypatch.setenv("CGEN_BLK3_FWD_PAIR", knob)
    monkeypatch.setenv("CGEN_BLK3_FWD_PAIR_SERIAL", serial)
    hp = _hp(kind)
    m = _model(hp)
    x, pa = _batch(hp)
    eng = m.engine()
    _seed(eng)
    l0 = eng.launches
    out = m(x, pa, beta=2.0)
    fwd, pairs = eng.launches - l0, eng.blk3_fwd_pairs
    assert not eng._blk3f.busy
    l1 = eng.launches
    out["elbo"].backward()
    bwd = eng.launches - l1
    torch.cuda.synchronize()
    vals = {k: out[k].detach().cpu().clone() for k in ("elbo", "nll", "kl")}
    grads = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters() if p.grad is not None}
    _seed(eng)
    with torch.no_grad():
        l2 = eng.launches
        zs = [z.detach().cpu().clone() for z in m.eval().abduct(x, pa)]
        abd, abd_pairs = eng.launches - l2, eng.blk3_fwd_pairs
    assert not eng._blk3f.busy
    return SimpleNamespace(vals=vals, grads=grads, zs=zs, fwd=fwd, bwd=bwd, pairs=pairs, abd=abd, abd_pairs=abd_pairs)


# (serial: the layers the pair does not serve -- 1 x 1, and 24 x 24 of "narrow" -- in line on the main stream, the default, or forked as before)
@pytest.mark.parametrize("kind,serial", [("narrow", "1"), ("narrow", "0"), ("wide", "1")])
def test_paired_forward_has_the_bits_and_one_launch_fewer_per_served_layer(monkeypatch, kind, serial):
    served = WIDTHS[kind][1]
    on, off = _one_pass(monkeypatch, "1", kind, serial), _one_pass(monkeypatch, "0", kind, serial)
    print("forward launches %d -> %d, backward %d -> %d, abduction %d -> %d" % (off.fwd, on.fwd, off.bwd, on.bwd, off.abd, on.abd))
    assert off.pairs == 0 and on.pairs == served, (off.pairs, on.pairs)
    assert off.fwd - on.fwd == served, (off.fwd, on.fwd)
    assert off.bwd == on.bwd, (off.bwd, on.bwd)
    for k in off.vals:
        assert torch.isfinite(off.vals[k]).all() and torch.equal(on.vals[k], off.vals[k]), (k, on.vals[k], off.vals[k])
    assert set(on.grads) == set(off.grads)
    for n in off.grads:
        assert torch.equal(on.grads[n], off.grads[n]), (n, float((on.grads[n].double() - off.grads[n].double()).abs().max()))
    # the non-recording abduction pass forks today (infer_branch): it takes the pair under the same rule
    assert off.abd_pairs == 0 and on.abd_pairs == served and off.abd - on.abd == served, (on.abd_pairs, off.abd, on.abd)
    assert len(on.zs) == len(off.zs) == 7
    for a, b in zip(on.zs, off.zs):
        assert torch.equal(a, b)


def test_three_graph_replayed_steps_equal_eager_and_the_two_queue_path(monkeypatch):
    from causal_gen_amd.train import TrainStep

    outs = {}
    for knob, use_graph in (("1", False), ("1", True), ("0", True)):
        monkeypatch.setenv("CGEN_BLK3_FWD_PAIR", knob)
        hp = _hp("wide", lr=2e-3, lr_warmup_steps=2)
        m = _model(hp)
        x, pa = _batch(hp)
        torch.manual_seed(123)
        ts = TrainStep(m, SimpleNamespace(**vars(hp)), ema=True, use_graph=use_graph)
        for _ in range(3):
            o = ts.step(x, pa)
        torch.cuda.synchronize()
        assert m.engine().blk3_fwd_pairs == (WIDTHS["wide"][1] if knob == "1" else 0)
        outs[(knob, use_graph)] = ([float(v) for v in o.cpu()], {k: v.clone() for k, v in m.state_dict().items()})
    o_ref, s_ref = outs[("1", True)]
    for key in (("1", False), ("0", True)):
        o, s = outs[key]
        assert o == o_ref, (key, o, o_ref)
        for k in s_ref:
            assert torch.equal(s[k], s_ref[k]), (key, k)
