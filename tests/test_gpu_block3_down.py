"""The encoder's down Block (vae.py:70-84: out = width_proj(x) + conv(x), avg_pool2d(out, 2)) inside the row-streaming launch of the
fused light Block (csrc/block.hip, blk3r_kernel<.., PROJ>; Engine.block2(proj=, down=), CGEN_BLK3_DOWN): forward -- projection,
residual add and 2x2 average in the Block's launch; backward -- the projection's data gradient in the Block's data-gradient launch.

Compared in one process against (a) the launches it replaces (projection conv, Block, pool; pool gradient, Block data gradient,
projection data gradient) -- same binary16 storage points, and the 1x1 sums formed as conv_px forms them: only where the separate
projection runs on another kernel (conv_smallp, up to 6 000 pixels) does a summation order differ -- and (b) torch f32 on the
f16-quantised operands.  Every arena tensor of a run sits between two guard bands that must come back untouched.

Served: 32 / 64 channels in, a bottleneck of 8 / 16, 32 / 64 out, on even images at least 48 wide and 16 high.  The 96-wide Block
(64 -> 16 -> 96: its instances need scratch registers, LABNOTES 25.4) and everything else (odd sides, a float down-rate) must be
DECLINED: the launches of before, bit for bit."""
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GUARD = 4096
PATTERN = 0x5A

# (N, H, W, ci, b, co)
SERVED = [
    (2, 16, 48, 32, 8, 64),   # the smallest served shape: two row strips of two bands, ragged second column strip (48 = 1.5 strips)
    (2, 20, 70, 32, 8, 64),   # ragged on both axes; the last band of a strip is partial; pooled width 35
    (3, 48, 96, 32, 8, 64),   # several strips both ways, more than one image per strip column
    (8, 96, 96, 32, 8, 64),   # the strip chooser takes 12-row strips here (288 eight-row strips would be two rounds): three bands per strip
    # the other widths of the row-streaming instance (each is a kernel instance of its own, forward and data gradient)
    (2, 16, 48, 32, 16, 64),  # 16-wide bottleneck; data gradient with a two-chunk ring
    (2, 20, 70, 64, 8, 32),   # two-chunk ring forward, one channel pair: waves 4-7 have no phase-B role; ragged
    (3, 48, 96, 64, 16, 32),  # the largest LDS footprint that fits (157 KB forward)
]
# (case, down-rate): the kernel or the engine declines -- today's launches, today's bits
DECLINED = [
    ((2, 17, 50, 32, 8, 64), 2),     # odd height
    ((2, 48, 48, 32, 8, 64), 2.0),   # a float down-rate (adaptive pooling)
    ((8, 96, 96, 64, 16, 96), 2),    # the 96-wide down Block: not on the row-streaming instance
    ((3, 24, 64, 64, 16, 96), 2),
]


class _Blk:
    """What vae.run_block reads of a Block."""

    def __init__(self, c1, c2, cp, d):
        self.light, self.residual, self.d, self.width_proj = True, True, d, cp
        self._cs = [c1, c2]

    def convs(self):
        return self._cs


_cache = {}


def _run(case, d, down):
    key = (case, d, down)
    if key in _cache:
        return _cache[key]
    from causal_gen_amd import vae
    from causal_gen_amd.engine import ConvSite, Engine

    N, H, W, ci, b, co = case
    g = torch.Generator().manual_seed(H * 7 + W + co)
    c1, c2, cp = torch.nn.Conv2d(ci, b, 3, padding=1), torch.nn.Conv2d(b, co, 3, padding=1), torch.nn.Conv2d(ci, co, 1)
    with torch.no_grad():
        c1.weight.copy_(torch.randn(c1.weight.shape, generator=g) / math.sqrt(ci * 9 / 2))
        c2.weight.copy_(torch.randn(c2.weight.shape, generator=g) / math.sqrt(b * 9 / 2))
        cp.weight.copy_(torch.randn(cp.weight.shape, generator=g) / math.sqrt(ci))
        c1.bias.copy_(torch.randn(b, generator=g) * 0.2)
        c2.bias.copy_(torch.randn(co, generator=g) * 0.2)
        cp.bias.copy_(torch.randn(co, generator=g) * 0.2)
    x = torch.randn(N, ci, H, W, generator=g).half().float()
    ho, wo = (int(W / d), int(W / d)) if isinstance(d, float) else (H // d, W // d)
    gout = torch.randn(N, co, ho, wo, generator=g).half().float()
    eng = Engine("cuda", "f16")
    eng.blk3_minres, eng.blk3_res, eng.blk3_res3 = 8, [], []
    holder = torch.nn.ModuleList([c1, c2, cp]).cuda()
    s1, s2 = ConvSite("c1", holder[0], [ci], [True], 0), ConvSite("c2", holder[1], [b], [True], 1)
    sp = ConvSite("proj", holder[2], [ci], [True], 2)
    s1.blk3, s2.blk3 = ("a", s2), ("b", s1)
    eng.blk3_on = 2
    eng.bind(holder, [s1, s2, sp])
    eng.blk3_down = down
    eng.begin()
    eng.prepare_weights(force=True)
    # ---- guard bands: the arena filled with a pattern, every allocation between two bands of it
    eng.arena.alloc(256)
    torch.cuda.synchronize()
    chunk = eng.arena.chunks[0]
    chunk.fill_(PATTERN)
    alloc0, bands = eng.arena.alloc, []

    def alloc(nbytes):
        p = alloc0(nbytes + 2 * GUARD)
        bands.append((p, nbytes))
        return p + GUARD

    eng.arena.alloc = alloc
    eng.recording = True
    xt = eng.from_nchw(x.cuda(), rg=True)
    n0 = eng.launches
    y = vae.run_block(eng, _Blk(holder[0], holder[1], holder[2], d), [xt])
    fwd_launches = eng.launches - n0
    assert (y.n, y.h, y.w, y.c) == (N, ho, wo, co)
    t = [a for fn, a, _ in eng.tape if fn == eng._bw_block3][0].mids[0]
    y_t, t_t = eng.to_nchw(y).cpu(), eng.to_nchw(t).cpu()
    gy = eng.seed_grad(y)
    eng.lib.axpby(eng.dt, N, ho, wo, eng.from_nchw(gout.cuda()).cv(), gy.cv(), 1.0, 1.0, 1 << 30, 0, eng.stream)
    eng.recording = False
    n1 = eng.launches
    eng.backward()
    bwd_launches = eng.launches - n1
    gx = eng.to_nchw(eng.grad_read(xt)).cpu()
    torch.cuda.synchronize()
    assert len(eng.arena.chunks) == 1
    base = chunk.data_ptr()
    for p, nbytes in bands:
        o = p - base
        lo, hi = chunk[o:o + GUARD], chunk[o + GUARD + nbytes:o + 2 * GUARD + nbytes]
        assert bool((lo == PATTERN).all()) and bool((hi == PATTERN).all()), ("guard band touched", nbytes)
    pg = [eng.param_grad_view(q).cpu().clone() for c in holder for q in (c.weight, c.bias)]
    out = dict(y=y_t, t=t_t, gx=gx, pg=pg, fwd=fwd_launches, bwd=bwd_launches, x=x, gout=gout, convs=(c1, c2, cp))
    _cache[key] = out
    return out


@pytest.mark.parametrize("case", SERVED, ids=["%d-%d-%d@%dx%d" % (c[3], c[4], c[5], c[1], c[2]) for c in SERVED])
def test_down_block_one_launch_against_the_three_and_torch(case):
    N, H, W, ci, b, co = case
    two = _run(case, 2, 0)
    one = _run(case, 2, 1)
    # forward: projection + Block + pool -> one launch; backward: the projection's data gradient is gone
    assert (two["fwd"], one["fwd"]) == (3, 1), (two["fwd"], one["fwd"])
    assert one["bwd"] == two["bwd"] - 1, (one["bwd"], two["bwd"])
    # ---- (a) against the launches of before
    assert torch.equal(one["t"], two["t"])  # the bottleneck: nothing about conv1 changed
    scale = float(two["y"].abs().max())
    dy = (one["y"] - two["y"]).abs()
    print("pooled output: max |d| %.3g of %.3g, %.3g %% of the elements differ" % (float(dy.max()), scale, 100 * float((dy > 0).float().mean())))
    assert float(dy.max()) <= 0.02 * scale and float((dy > 0).float().mean()) < 0.05, (float(dy.max()), scale, float((dy > 0).float().mean()))
    a, c = one["gx"], two["gx"]
    print("grad(x): max |d| %.3g of %.3g, norm %.3g of %.3g" % (float((a - c).abs().max()), float(c.abs().max()), float((a - c).norm()), float(c.norm())))
    assert float((a - c).abs().max()) <= 0.03 * float(c.abs().max())
    assert float((a - c).norm()) <= 5e-3 * float(c.norm())
    for a, c in zip(one["pg"], two["pg"]):
        assert float((a - c).norm()) <= 1e-2 * float(c.norm()) + 1e-6, (float((a - c).norm()), float(c.norm()))
    # ---- (b) against torch f32 on the same f16-quantised operands
    c1, c2, cp = one["convs"]
    w1, w2, wp = [m.weight.detach().cpu().half().float().requires_grad_(True) for m in (c1, c2, cp)]
    xr = one["x"].clone().requires_grad_(True)
    tt = F.conv2d(F.relu(xr), w1, c1.bias.detach().cpu(), padding=1)
    y = F.conv2d(F.relu(tt), w2, c2.bias.detach().cpu(), padding=1) + F.conv2d(xr, wp, cp.bias.detach().cpu())
    y = F.avg_pool2d(y, 2)
    y.backward(one["gout"])
    torch.testing.assert_close(one["y"], y.detach(), rtol=3e-2, atol=3e-2)
    assert float((one["gx"] - xr.grad).norm()) <= 2e-2 * float(xr.grad.norm())
    for k, w in ((0, w1), (2, w2), (4, wp)):
        assert float((one["pg"][k] - w.grad).norm()) <= 3e-2 * float(w.grad.norm()), k


@pytest.mark.parametrize("case,d", DECLINED, ids=["%dx%dx%d-d%s" % (c[1], c[2], c[5], d) for c, d in DECLINED])
def test_declined_shapes_run_the_launches_of_before_bit_for_bit(case, d):
    two = _run(case, d, 0)
    one = _run(case, d, 1)
    assert (one["fwd"], one["bwd"]) == (two["fwd"], two["bwd"])
    for k in ("y", "t", "gx"):
        assert torch.equal(one[k], two[k]), k
    for a, c in zip(one["pg"], two["pg"]):
        assert torch.equal(a, c)


# ----------------------------------------------------------------------------- model level
def _hp(**over):
    from causal_gen_amd.hps import setup_hparams

    # the encoder's first down Block is 32 -> 8 -> 64 on 48 x 48: served; the others (24 x 24 and below) are not.  Batch 3: 6 912 pixels,
    # so that the 1x1 projection of the unfused path runs on conv_px, the kernel it runs on at the flagship size and whose arithmetic
    # (v_mfma_f32_16x16x32, 32 channels per step, the bias as the initial value) the fused launch repeats.  Up to 6 000 pixels the
    # unfused projection is conv_smallp's, with another summation order: the kernel-level cases above cover that pairing.
    return setup_hparams("ukbb192", input_res=48, enc_arch="48b1d2,24b1d2,12b1d2,6b1d6,1b1", dec_arch="1b1,6b1,12b1,24b1,48b1",
                         widths=[32, 64, 96, 128, 160], z_max_res=24, z_dim=8, bs=3, **over)


def _model(hp):
    from causal_gen_amd import vae

    torch.manual_seed(7)
    m = vae.HVAE(hp)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for p in m.parameters():  # (the reference zero-initialises the prior heads: every conv gets weight)
            p.add_(torch.randn(p.shape, generator=g) * 0.05)
    m.compute_dtype = "f16"
    return m.cuda().train()


def _batch(hp, B=3):
    g = torch.Generator().manual_seed(1)
    R = hp.input_res
    x = (torch.randint(0, 256, (B, 1, R, R), generator=g).float() - 127.5) / 127.5
    pa = torch.randn(B, hp.context_dim, generator=g)
    return x.cuda(), pa.cuda()[..., None, None].expand(-1, -1, R, R)


def _pass(monkeypatch, knob):
    monkeypatch.setenv("CGEN_BLK3_DOWN", knob)
    hp = _hp()
    m = _model(hp)
    x, pa = _batch(hp)
    eng = m.engine()
    eng.rng_ptr()
    eng.rng.copy_(torch.tensor([11, 0], dtype=torch.int64, device=eng.rng.device))
    l0 = eng.launches
    out = m(x, pa, beta=2.0)
    fwd = eng.launches - l0
    l1 = eng.launches
    out["elbo"].backward()
    bwd = eng.launches - l1
    torch.cuda.synchronize()
    vals = {k: float(out[k].detach().cpu()) for k in ("elbo", "nll", "kl")}
    grads = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters() if p.grad is not None}
    return vals, grads, fwd, bwd


def test_model_knob_on_against_off(monkeypatch):
    """ELBO, NLL and KL to 1e-4 relative (the project's parity bound), every parameter gradient to 1e-2 of its norm; two launches
    fewer forward and one fewer backward (one served down Block)."""
    v1, g1, f1, b1 = _pass(monkeypatch, "1")
    v0, g0, f0, b0 = _pass(monkeypatch, "0")
    print("launches forward %d -> %d, backward %d -> %d" % (f0, f1, b0, b1), v0, v1)
    assert f0 - f1 == 2 and b0 - b1 == 1, (f0, f1, b0, b1)
    for k in v0:
        assert abs(v1[k] - v0[k]) <= 1e-4 * abs(v0[k]), (k, v1[k], v0[k])
    assert set(g1) == set(g0)
    print("parameter gradients with other bits:", sorted(n for n in g0 if not torch.equal(g1[n], g0[n])))
    for n in g0:
        assert float((g1[n] - g0[n]).norm()) <= 1e-2 * float(g0[n].norm()), (n, float((g1[n] - g0[n]).norm()), float(g0[n].norm()))


def test_train_step_graph_replay_equals_eager_with_the_knob_on(monkeypatch):
    from causal_gen_amd.train import TrainStep

    monkeypatch.setenv("CGEN_BLK3_DOWN", "1")
    outs = []
    for use_graph in (False, True):
        hp = _hp(lr=2e-3, lr_warmup_steps=2)
        m = _model(hp)
        x, pa = _batch(hp)
        torch.manual_seed(123)
        ts = TrainStep(m, SimpleNamespace(**vars(hp)), ema=True, use_graph=use_graph)
        for _ in range(3):
            o = ts.step(x, pa)
        torch.cuda.synchronize()
        outs.append(([float(v) for v in o.cpu()], {k: v.clone() for k, v in m.state_dict().items()}))
    (o0, s0), (o1, s1) = outs
    assert o0 == o1, (o0, o1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
