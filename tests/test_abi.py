"""The C-ABI library loads without a GPU and exports every symbol include/cgen_hip.h declares; the ctypes binding
covers exactly that set (what it binds them AS -- structs, constants, argument types: tests/test_abi_mirror.py); the host-side
plan queries and argument checks answer without a GPU; the shipped code objects keep the packed-f32 ban and their scratch budget."""
import ctypes
import os
import re

from conftest import ROOT


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "cgen_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(cgen_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported_and_bound():
    from causal_gen_amd import _lib

    lib = _lib.load()
    syms = declared_symbols()
    assert len(syms) >= 35
    for s in syms:
        assert hasattr(lib.cdll, s), f"{s} declared in cgen_hip.h but not exported by libcgen_hip.so"
    assert sorted(_lib.PROTOTYPES) == syms
    assert lib.version() >= 100
    assert lib.last_error() is not None


def test_wgrad_plan_and_record_without_gpu():
    from causal_gen_amd import _lib

    lib = _lib.load()
    w = _lib.WgradArgs()
    w.dtype, w.n, w.h, w.w, w.ks, w.nseg = 1, 32, 192, 192, 3, 1
    w.seg[0] = _lib.View(4096, 192 * 192 * 32, 192 * 32, 32, 32, 0)
    w.gout = _lib.View(8192, 192 * 192 * 8, 192 * 8, 8, 8, 0)
    tiled = ctypes.c_int32(-1)
    # 32 -> 8 channels, 3x3: the streaming kernel (round 5) takes it with grad_out (the narrow operand) as the shifted one => layout 1
    assert lib.conv2d_wgrad_plan(ctypes.byref(w), ctypes.byref(tiled)) >= 1 and tiled.value == 3
    w.seg[0], w.gout = _lib.View(8192, 192 * 192 * 8, 192 * 8, 8, 8, 0), _lib.View(4096, 192 * 192 * 32, 192 * 32, 32, 32, 0)
    assert lib.conv2d_wgrad_plan(ctypes.byref(w), ctypes.byref(tiled)) >= 1 and tiled.value == 2  # 8 -> 32: X is the narrow operand
    w.ks = 7  # the 7x7 stem (one input channel, zero padded to 8): X is the shifted operand, 49 taps x 8 = 13 fragments
    w.seg[0] = _lib.View(4096, 192 * 192 * 8, 192 * 8, 8, 1, 8)
    assert lib.conv2d_wgrad_plan(ctypes.byref(w), ctypes.byref(tiled)) >= 1 and tiled.value == 2
    w.dtype = 0  # f32: the generic kernel
    assert lib.conv2d_wgrad_plan(ctypes.byref(w), ctypes.byref(tiled)) >= 1 and tiled.value == 0
    # cgen_conv2d_wgrad_plan_record is host code: what cgen_conv2d_wgrad_plan answers, and the record the launch is made from
    rec = (ctypes.c_int32 * _lib.WGRAD_PLAN_INTS)(*([-1] * _lib.WGRAD_PLAN_INTS))
    w.partial_b = None
    assert lib.conv2d_wgrad_plan_record(ctypes.byref(w), rec) == lib.conv2d_wgrad_plan(ctypes.byref(w), None) == rec[1]
    # wgrad_kernel<float, 2>: 32 channels = one chunk, 49 taps = six groups, vector loads on both sides, no bias partial
    assert tuple(rec[:10]) == (0, rec[1], 0, 2, 1, 6, rec[6], 1, 1, 0) and rec[6] % 64 == 0 and not any(rec[10:])
    w.partial_b = 4096
    assert lib.conv2d_wgrad_plan_record(ctypes.byref(w), rec) == rec[1] and rec[9] == 1
    w.dtype, w.ks = 1, 3  # 16-bit 3x3, 256 -> 256 on dense views: wgrad_tile_kernel<4, 6, 3>, windows of 32 channels, one tile buffer
    w.n, w.h, w.w = 2, 6, 6
    w.seg[0] = w.gout = _lib.View(4096, 6 * 6 * 256, 6 * 256, 256, 256, 0)
    assert lib.conv2d_wgrad_plan_record(ctypes.byref(w), rec) == rec[1] == 1
    assert tuple(rec[:13]) == (1, 1, 4, 6, 3, 32, 8, 4, 2, 2, 0, 45056, 9) and not any(rec[13:])
    w.seg[0] = w.gout = _lib.View(4096, 6 * 6 * 128, 6 * 128, 128, 128, 0)  # 128 -> 128: the streaming kernel, nothing beyond kind and nsplit
    assert lib.conv2d_wgrad_plan_record(ctypes.byref(w), rec) == rec[1] and rec[0] == 2 and not any(rec[2:])
    w.nseg = 0
    rec[0] = -7
    assert lib.conv2d_wgrad_plan_record(ctypes.byref(w), rec) == 0 and rec[0] == -7  # (bad arguments: out[] untouched)


def test_block3_plan_without_gpu():
    """cgen_block3_plan is host code: what cgen_block3_supported answers, and the record the launch is made from"""
    from causal_gen_amd import _lib

    lib = _lib.load()
    blk = _lib.Block3Args()
    blk.dtype, blk.n, blk.h, blk.w, blk.nseg, blk.nout, blk.pre_act = _lib.F16, 2, 24, 24, 1, 1, 1
    blk.seg[0] = _lib.View(1 << 20, 24 * 24 * 128, 24 * 128, 128, 128, 0)
    blk.w_a, blk.mid = 1 << 20, _lib.View(1 << 20, 24 * 24 * 32, 24 * 32, 32, 32, 0)
    blk.o[0].w, blk.o[0].out = 1 << 20, _lib.View(1 << 20, 24 * 24 * 160, 24 * 160, 160, 160, 0)
    rec = (ctypes.c_int32 * _lib.BLOCK3_PLAN_INTS)(*([-1] * _lib.BLOCK3_PLAN_INTS))
    assert lib.block3_plan(ctypes.byref(blk), rec) == lib.block3_supported(ctypes.byref(blk)) == 1
    assert tuple(rec[:7]) == (0, 1, 4, 4, 0, 8, 0) and (rec[7], rec[9], rec[10]) == (3, 12, 12) and not any(rec[19:])  # blk3_kernel<true, 4, 4, 0, 8, false>
    blk.h = 3
    assert lib.block3_plan(ctypes.byref(blk), rec) == 0 and lib.block3_plan(ctypes.byref(blk), None) == 0 and rec[0] == 0  # (declined: out[] untouched)


def test_block4_plan_without_gpu():
    """cgen_block4_plan likewise: blk4_kernel<true, 2, 8>, 18 tiles of 8 x 16, four chunks of 32 input channels"""
    from causal_gen_amd import _lib

    lib = _lib.load()
    b4 = _lib.Block4Args()
    b4.dtype, b4.n, b4.h, b4.w, b4.nseg, b4.nout, b4.fwd, b4.b = _lib.F16, 2, 24, 40, 1, 1, 1, 16
    b4.seg[0] = _lib.View(1 << 20, 24 * 40 * 128, 40 * 128, 128, 128, 0)
    for k in range(3):
        b4.wimg[k], b4.mid[k] = 1 << 20, _lib.View(1 << 20, 24 * 40 * 16, 40 * 16, 16, 16, 0)
    b4.o[0].w, b4.o[0].out = 1 << 20, _lib.View(1 << 20, 24 * 40 * 64, 40 * 64, 64, 64, 0)
    rec = (ctypes.c_int32 * _lib.BLOCK4_PLAN_INTS)(*([-1] * _lib.BLOCK4_PLAN_INTS))
    assert lib.block4_plan(ctypes.byref(b4), rec) == lib.block4_supported(ctypes.byref(b4)) == 1
    assert tuple(rec[:5]) == (1, 2, 8, 18, 18) and tuple(rec[6:10]) == (0, 3, 3, 4) and not any(rec[10:])
    b4.b = 56
    assert lib.block4_plan(ctypes.byref(b4), rec) == 0 and lib.block4_plan(ctypes.byref(b4), None) == 0 and rec[0] == 1  # (declined: out[] untouched)


def test_predictor_tiled_plan_without_gpu():
    """cgen_predictor_tiled_plan is host code: the 13 launches of the tiled placement, read from the functions the launchers read.
    ukbb192 (1 x 192 x 192, width 16, 4 heads, B = 32): stride-2 stem, the pool inside layer 1, 16-pixel tiles down to 24 x 24"""
    from causal_gen_amd import _lib

    lib = _lib.load()
    hd = (_lib.PredHead * 4)()
    for h in hd:
        h.c, h.res, h.width, h.nout, h.kind, h.obs_stride = 1, 192, 16, 2, _lib.PRED_NORMAL, 1
    ints = _lib.PRED_PLAN_FIELDS * _lib.PRED_PLAN_LAUNCHES
    prec = (ctypes.c_int32 * ints)(*([-1] * ints))
    cnt = ctypes.c_int32(0)
    lib.predictor_tiled_plan(hd, 4, 32, prec, _lib.PRED_PLAN_LAUNCHES, ctypes.byref(cnt))
    assert cnt.value == 13
    got = [tuple(prec[8 * i:8 * i + 8]) for i in range(13)]
    assert got[0] == (0, 7, 2, 2, 4, 0, 0, 128 * 36) and got[1] == (0, 3, 2, 2, 8, 1, 1, 128 * 4)  # ptile_conv_fwd<7,2,2,4,false>, <3,2,2,8,true>
    assert got[6] == (3, 0, 0, 0, 0, 0, 6, 128) and got[7] == (1, 3, 2, 0, 8, 0, 5, 128 * 2 * 1)   # ptile_tail, ptile_conv_bwd<2,8,0>
    assert got[11] == (1, 3, 2, 0, 4, 1, 1, 128 * 9) and got[12] == (2, 7, 2, 0, 0, 0, 0, 32 * 36)  # ptile_conv_bwd<2,4,1>, ptile_stem_bwd<2>
    hd[1].width = 8  # unequal widths: refused, the records untouched
    prec[0] = -7
    assert lib._raw_cgen_predictor_tiled_plan(hd, 4, 32, prec, _lib.PRED_PLAN_LAUNCHES, ctypes.byref(cnt)) != 0 and prec[0] == -7


def test_pure_queries_and_conv2d_validation_without_gpu():
    from causal_gen_amd import _lib

    lib = _lib.load()
    assert lib.reparam_kl_chunks(96, 96, 16) == 72
    assert lib.like_chunks(192, 192) == 36
    last = lib.conv2d_last_kernel()  # "" until a conv has been launched in this thread (a CPU-only host cannot launch one)
    assert last in (b"", b"gen", b"tile", b"px", b"ws", b"smlp", b"smlp2")
    # argument validation happens before any launch, so it is testable on a CPU-only host
    a = _lib.ConvArgs()
    a.dtype = 7
    try:
        lib.conv2d(ctypes.byref(a), None)
        raise AssertionError("expected CgenError")
    except _lib.CgenError as e:
        assert "dtype" in str(e)
    assert lib.conv2d_last_kernel() == last  # (a call that is refused serves nothing)


def test_product_path_fails_loudly_without_gpu():
    import pytest
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from causal_gen_amd import _lib, vae
    from causal_gen_amd.hps import setup_hparams

    m = vae.HVAE(setup_hparams("morphomnist"))
    x = torch.zeros(1, 1, 32, 32)
    pa = torch.zeros(1, 12, 32, 32)
    with pytest.raises(_lib.CgenError):
        m(x, pa)
    with pytest.raises(RuntimeError):
        m.encoder(x)  # holders never compute


def test_device_code_has_no_packed_f32_instructions():
    """MI355X erratum found in round 1 (tools/coexec_probe.py): v_pk_mul/add/fma_f32 in one wave return
    corrupted results while a wave of ANOTHER kernel on the same SIMD executes a 16-bit MFMA (found with v_mfma_f32_16x16x32_bf16; the f16 build keeps the guard) -- the background
    weight-gradient kernel runs next to the whole backward chain.  build.sh switches the packed-fp32 feature off; this
    checks the shipped library instead of the flag."""
    import subprocess

    import codeobj

    bundles = codeobj.bundle_paths()
    assert bundles, "no gfx950 code object in the library"
    n_inst = 0
    for b in bundles:
        asm = subprocess.run([codeobj.OBJDUMP, "-d", b], check=True, capture_output=True, text=True).stdout
        n_inst += asm.count("v_mfma_f32_16x16x32_f16") + asm.count("v_mfma_f32_16x16x32_bf16")
        bad = re.findall(r"v_pk_(?:mul|add|fma)_f32", asm)
        assert not bad, "%d packed-f32 instructions in %s" % (len(bad), os.path.basename(b))
    assert n_inst > 0  # we did look at the real kernels


def test_hand_scheduled_kernels_keep_their_scratch_budget():
    """the fused Block kernel (csrc/block.hip) and the streaming weight-gradient kernel (csrc/wgrad3.hip) order their
    untracked LDS-DMA requests by counted `s_waitcnt vmcnt(N)`.  A compiler-made VMEM operation (a scratch access) between them
    cannot break that -- requests retire in order, so an extra counted operation only makes a wait cover MORE of the older
    requests -- but it costs time on the chain, and a spill inside a tile loop would be a performance bug nobody sees.  This pins
    the state of the shipped library: every blk3 instance has its 20-byte private array (5 dwords, indexed dynamically) and
    nothing else, except four instances with 8-14 spilled registers (three remainder-plane ones, one streaming data-gradient
    one); the weight-gradient kernels keep at most a handful of COLD values (entry / epilogue) in scratch.  Growth fails here."""
    import codeobj

    seen = {"blk3": 0, "wg3": 0}
    spilling = []
    for name, scratch, spills in codeobj.kernels():
        if "blk3_kernel" in name:
            seen["blk3"] += 1
            assert scratch <= 80 and spills <= 16, (name, scratch, spills)
            if spills:
                spilling.append(name)
        if "wg3_" in name:
            seen["wg3"] += 1
            assert scratch <= 64 and spills <= 8, (name, scratch, spills)
    assert seen["blk3"] >= 10 and seen["wg3"] >= 2, seen
    assert len(spilling) <= 4, spilling
