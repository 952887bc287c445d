"""The DMoL decode backward entry points without a GPU: argument validation happens before any launch, and the gfx950 code
object holds both storage instances of the two new kernels with no scratch and no spilled registers."""
import re

import pytest

import codeobj


def _view(c):
    from causal_gen_amd import _lib

    # a fake device address: validation must reject the call before anything dereferences it
    return _lib.View(4096, 8 * 8 * c, 8 * c, c, c, 0)


def _decode_bwd(lib, mode=0, c=100, rng=True):
    from causal_gen_amd import _lib

    return lib._raw_cgen_dmol_decode_bwd(_lib.F32, 2, 8, 8, _view(c), mode, 8192 if rng else None, 977, 0.0, 12288, None, 1.0,
                                         _view(100), None)


def _cf_bwd(lib, mode=0, c=100):
    from causal_gen_amd import _lib

    return lib._raw_cgen_cf_dmol_bwd(_lib.F32, 2, 8, 8, mode, _view(c), _view(100), _view(3), 12288, 1.0, _view(100), _view(c), None)


def test_dmol_backward_entry_points_reject_bad_arguments():
    from causal_gen_amd import _lib

    lib = _lib.load()
    cases = [
        (lambda: _decode_bwd(lib, mode=3), "bad mode 3"),
        (lambda: _decode_bwd(lib, mode=10), "bad mode 10"),
        (lambda: _decode_bwd(lib, mode=20), "bad mode 20"),
        (lambda: _decode_bwd(lib, c=99), "100 channels"),
        (lambda: _decode_bwd(lib, mode=2, rng=False), "rng"),
        (lambda: _cf_bwd(lib, mode=2), "bad mode 2"),
        (lambda: _cf_bwd(lib, mode=7), "bad mode 7"),
        (lambda: _cf_bwd(lib, c=64), "100 channels"),
    ]
    for call, words in cases:
        rc = call()
        assert rc < 0, words
        msg = lib.last_error().decode()
        assert words in msg, (words, msg)
    # and through the checked binding
    with pytest.raises(_lib.CgenError, match="cgen_cf_dmol_bwd"):
        lib.cf_dmol_bwd(_lib.F32, 2, 8, 8, 5, _view(100), _view(100), _view(3), 12288, 1.0, _view(100), _view(100), None)


def test_dmol_backward_kernels_have_no_scratch_and_no_spills():
    seen = {}
    for name, scratch, spills in codeobj.kernels():
        k = re.search(r"(dmol_decode_bwd_kernel|cf_dmol_bwd_kernel)I([ft])", name)
        if not k:
            continue
        seen[k.group(1) + ("<float>" if k.group(2) == "f" else "<h16_t>")] = name
        assert scratch == 0, (name, scratch)
        assert spills == 0, (name, spills)
    assert sorted(seen) == ["cf_dmol_bwd_kernel<float>", "cf_dmol_bwd_kernel<h16_t>", "dmol_decode_bwd_kernel<float>",
                            "dmol_decode_bwd_kernel<h16_t>"], sorted(seen)
