"""The device-resident input pipeline without a GPU: the entry point is exported and bound at ABI 411, every argument check runs
before any launch, the case table of tests/test_gpu_augment.py reaches every store arm, and the host-side logic of
causal_gen_amd.data (per-preset geometry as src/datasets.py + hps.py give it, loader sharding) is right."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest
import torch

from augment_cases import CASES, GEOMS, arm_of
from conftest import ROOT


def _args(**kw):
    from causal_gen_amd import _lib

    a = _lib.AugmentArgs()
    a.dtype, a.n, a.c, a.h0, a.w0, a.r_h, a.r_w, a.pad_x, a.pad_y, a.ctx = _lib.F32, 2, 1, 28, 28, 32, 32, 4, 4, 0
    a.stream_id, a.hflip_p, a.sub, a.mul, a.n_data = _lib.STREAM_AUGMENT, 0.5, 127.5, 1 / 127.5, 10
    # fake device addresses: validation must reject before anything dereferences them or is launched
    a.data, a.index, a.rng = 4096, 8192, 12288
    a.out = _lib.View(16384, 32 * 32, 32, 1, 1, 0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_symbol_exported_declared_and_abi_411():
    from causal_gen_amd import _lib

    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "cgen_hip.h")).read()
    assert re.search(r"int cgen_batch_augment\(const cgen_augment_args\* a, cgen_stream_t stream\);", hdr)
    assert "#define CGEN_ABI_VERSION 411" in hdr
    assert hasattr(lib.cdll, "cgen_batch_augment") and "cgen_batch_augment" in _lib.PROTOTYPES
    assert lib.version() == 411 == _lib.ABI_VERSION
    assert _lib.STREAM_AUGMENT == 980
    common = open(os.path.join(ROOT, "causal-gen_amd", "csrc", "common.h")).read()
    assert "#define CGEN_STREAM_AUGMENT 980u" in common and all(f"//   {i} " in common for i in (977, 978, 979, 980))


def test_validation_rejects_before_any_launch():
    from causal_gen_amd import _lib

    lib = _lib.load()
    V = _lib.View
    cases = [
        (_args(data=None), "null data, index or out"),
        (_args(index=None), "null data, index or out"),
        (_args(out=V(None, 1024, 32, 1, 1, 0)), "null data, index or out"),
        (_args(n=0), "empty batch"),
        (_args(n=-3), "empty batch"),
        (_args(c=0, out=V(16384, 1024, 32, 1, 0, 0)), "c must be 1..4"),
        (_args(c=5, out=V(16384, 5 * 1024, 5 * 32, 5, 5, 0)), "c must be 1..4"),
        (_args(r_h=37), "larger than the padded image"),
        (_args(r_w=37), "larger than the padded image"),
        (_args(hflip_p=-0.01), "outside [0, 1]"),
        (_args(hflip_p=1.5), "outside [0, 1]"),
        (_args(hflip_p=float("nan")), "outside [0, 1]"),
        (_args(out=V(16384, 3 * 1024, 3 * 32, 3, 3, 0)), "out.c 3 != c 1"),
        (_args(dtype=_lib.F32S), "bad dtype"),
        (_args(dtype=7), "bad dtype"),
        (_args(pa_out=4096), "go together"),
        (_args(pa_data=4096), "go together"),
        (_args(pa_data=4096, pa_out=20480, ctx=0), "ctx must be > 0"),
        (_args(pa_data=4096, pa_out=20480, ctx=-2), "ctx must be > 0"),
        (_args(rng=None), "neither a Philox state nor injected draws"),
    ]
    for a, words in cases:
        assert lib._raw_cgen_batch_augment(C.byref(a), None) < 0, words
        msg = lib.last_error().decode()
        assert words in msg, (words, msg)
        assert lib.batch_augment_arm(C.byref(a)) < 0, words
    with pytest.raises(_lib.CgenError, match="cgen_batch_augment"):
        lib.batch_augment(C.byref(_args(c=9)), None)
    assert lib.batch_augment_arm(C.byref(_args())) == 0  # the good record plans (nothing is launched by the query)
    assert lib.batch_augment_arm(C.byref(_args(rng=None, draws_in=4096))) == 0


def test_gpu_case_table_reaches_every_store_arm():
    """arm_of() asks the library which kernel instance a case's output view takes (0 / 1 / 2: contiguous rows, all 16-byte stores /
    16-byte stores + element-wise row end / element-wise; 3 / 4: one padded pixel per lane, 16-byte / element-wise)."""
    seen = {(dt, arm_of(cs, dt)) for cs in CASES for dt in ("f32", "h16")}
    assert seen == {(dt, arm) for dt in ("f32", "h16") for arm in range(5)}, sorted(seen)
    # the issue's geometries are all in the table, with both channel counts
    assert {(cs.c,) + cs.geom for cs in CASES} >= {(c,) + g for c in (1, 3) for g in GEOMS}
    odd = [cs for cs in CASES if cs.geom == (9, 13, 9, 13, 3, 2) and cs.layout == "packed"]
    assert odd and all(arm_of(cs, dt) == 2 for cs in odd for dt in ("f32", "h16"))  # odd r_w * c: element-wise rows


def _hp(name, **kw):
    from causal_gen_amd.hps import setup_hparams

    return setup_hparams(name, **kw)


def test_from_args_geometry_of_the_four_presets():
    """Written out by hand from the reference: hps.py ukbb192.pad = 9, morphomnist.pad = cmnist.pad = 4, --hflip default 0.5;
    datasets.py ukbb RandomCrop(padding=[2 * pad, pad]) + RandomHorizontalFlip(hflip), MNIST RandomCrop(32, padding=pad) and no
    flip, eval Pad(2); mimic Resize only."""
    from causal_gen_amd import DeviceDataset

    def mk(name, c, h0, ctx):
        return DeviceDataset.from_args(_hp(name), torch.zeros(3, c, h0, h0, dtype=torch.uint8), torch.zeros(3, ctx), device="cpu")

    u = mk("ukbb192", 1, 192, 4)
    assert u.geometry(True) == (192, 192, 18, 9, 0.5) and u.draw_range(True) == (18, 36)
    assert u.geometry(False) == (192, 192, 0, 0, 0.0) and u.draw_range(False) == (0, 0)  # evaluation: the identity
    for name, c, ctx in (("morphomnist", 1, 12), ("cmnist", 3, 20)):
        m = mk(name, c, 28, ctx)
        assert (m.h0, m.r_h) == (28, 32)
        assert m.geometry(True) == (32, 32, 4, 4, 0.0) and m.draw_range(True) == (4, 4)
        assert m.geometry(False) == (32, 32, 2, 2, 0.0) and m.draw_range(False) == (0, 0)  # Pad(2)
    for name, r in (("mimic192", 192), ("mimic224", 224)):
        k = mk(name, 1, r, 6)
        assert k.geometry(True) == (r, r, 0, 0, 0.0) and k.draw_range(True) == (0, 0)
    with pytest.raises(ValueError, match="no augmentation recipe"):
        DeviceDataset.from_args(SimpleNamespace(hps="celeba", input_res=8), torch.zeros(1, 1, 8, 8, dtype=torch.uint8), torch.zeros(1, 1),
                                device="cpu")
    with pytest.raises(ValueError, match="does not fit"):
        DeviceDataset(torch.zeros(1, 1, 8, 8, dtype=torch.uint8), torch.zeros(1, 1), 12, pad=(1, 2), device="cpu")
    small = DeviceDataset(torch.zeros(1, 1, 8, 8, dtype=torch.uint8), torch.zeros(1, 1), 6, pad=(0, 0), device="cpu")
    with pytest.raises(ValueError, match="evaluation pads"):
        small.geometry(False)  # R < h0: evaluation cannot crop


def test_loader_shards_one_shared_permutation():
    from causal_gen_amd import DeviceDataset, DeviceLoader

    n, bs = 50, 6
    ds = DeviceDataset(torch.zeros(n, 1, 4, 4, dtype=torch.uint8), torch.zeros(n, 2), 4, device="cpu")
    loaders = [DeviceLoader(ds, bs, generator=torch.Generator().manual_seed(5), rank=r, world_size=2) for r in (0, 1)]
    assert len(loaders[0]) == len(loaders[1]) == n // (2 * bs) == 4
    for epoch in range(2):
        shards = [list(ld.indices()) for ld in loaders]
        assert torch.equal(loaders[0].last_perm, loaders[1].last_perm)
        perm = loaders[0].last_perm
        assert sorted(perm.tolist()) == list(range(n))
        assert all(len(s) == 4 and all(i.numel() == bs and i.dtype == torch.int64 for i in s) for s in shards)
        a, b = (set(torch.cat(s).tolist()) for s in shards)
        assert not (a & b) and len(a) == len(b) == 4 * bs
        assert a | b == set(perm[:2 * bs * 4].tolist())  # drop_last: the tail of the permutation sits this epoch out
        for step in range(4):  # each global batch is one contiguous slice of the permutation, rank r its r-th half
            assert torch.equal(torch.cat([shards[0][step], shards[1][step]]), perm[step * 2 * bs:(step + 1) * 2 * bs])
        if epoch == 0:
            first = perm.clone()
    assert not torch.equal(first, loaders[0].last_perm)  # a fresh permutation per epoch
    # one rank, no shuffle, keep the tail
    ld = DeviceLoader(ds, 8, shuffle=False, drop_last=False)
    got = list(ld.indices())
    assert len(ld) == len(got) == 7 and torch.equal(torch.cat(got), torch.arange(n)) and got[-1].numel() == 2
    n48 = DeviceDataset(torch.zeros(48, 1, 4, 4, dtype=torch.uint8), torch.zeros(48, 2), 4, device="cpu")
    both = [torch.cat(list(DeviceLoader(n48, bs, generator=torch.Generator().manual_seed(1), rank=r, world_size=2).indices())) for r in (0, 1)]
    assert sorted(torch.cat(both).tolist()) == list(range(48))  # divisible: the two ranks together are the permutation
    with pytest.raises(ValueError, match="drop_last"):
        DeviceLoader(ds, bs, drop_last=False, world_size=2)
