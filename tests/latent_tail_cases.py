"""What the three latent-tail GPU test files (tests/test_gpu_latent_tail.py, _fwd.py, _det.py) share: the weight images of
cgen_weight_prep for a 1x1 conv built on the CPU, and the small weight-perturbed HVAE, its batch, its Philox seed and the bit-for-bit
comparison of two passes that their model-level tests use.  The Case classes, the hyper-parameters of the small model (`_small_hp`:
they differ on purpose) and every parametrisation stay with the tests."""
import torch


def _lib():
    from causal_gen_amd import _lib

    return _lib


def _ceil(a, m):
    return (a + m - 1) // m * m


def _fwd_image(w16, seg_c):
    """cgen_weight_prep mode 0 for a 1x1 conv, from the binary16-rounded OI weights: row = output channel, column = position in the
    concatenation of the input segments, each padded to 8 channels; rows padded to 16, ceil32(columns) + 32 columns."""
    co = w16.shape[0]
    k8 = sum(_ceil(c, 8) for c in seg_c)
    img = torch.zeros(_ceil(co, 16), _ceil(k8, 32) + 32, dtype=torch.float16)
    src = dst = 0
    for c in seg_c:
        img[:co, dst:dst + c] = w16[:, src:src + c]
        src, dst = src + c, dst + _ceil(c, 8)
    return img


def _dgrad_image(w16, seg_off, seg_c):
    """cgen_weight_prep mode 1 for a 1x1 conv, from the binary16-rounded OI weights: img[r][k] = W[k][seg_off + r]."""
    co = w16.shape[0]
    img = torch.zeros(_ceil(seg_c, 16), _ceil(_ceil(co, 8), 32) + 32, dtype=torch.float16)
    img[:seg_c, :co] = w16[:, seg_off:seg_off + seg_c].t()
    return img


def _small_model(hp, dtype="f16"):
    from causal_gen_amd import vae

    torch.manual_seed(7)
    m = vae.HVAE(hp)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for p in m.parameters():  # (the reference zero-initialises the prior heads: every conv gets weight)
            p.add_(torch.randn(p.shape, generator=g) * 0.05)
    m.compute_dtype = dtype
    return m.cuda().train()


def _batch(hp, B):
    g = torch.Generator().manual_seed(1)
    R = hp.input_res
    x = (torch.randint(0, 256, (B, 1, R, R), generator=g).float() - 127.5) / 127.5
    pa = torch.randn(B, hp.context_dim, generator=g)
    return x.cuda(), pa.cuda()[..., None, None].expand(-1, -1, R, R)


def _seed(eng):
    eng.rng_ptr()
    eng.rng.copy_(torch.tensor([11, 0], dtype=torch.int64, device=eng.rng.device))


def _same(a, b):
    """(values, gradients) of two passes: equal bits, the same set of gradients."""
    (v1, g1), (v0, g0) = a, b
    for k in v0:
        assert torch.equal(v1[k], v0[k]), (k, v1[k], v0[k])
    assert set(g1) == set(g0)
    for n in g0:
        assert torch.equal(g1[n], g0[n]), (n, float((g1[n].double() - g0[n].double()).abs().max()))
