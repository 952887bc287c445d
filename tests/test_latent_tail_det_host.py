"""Engine._latent_tail_at on hand-built tapes (no launch, no GPU): the deterministic form of a decoder layer's tail -- z_proj reading
the slice [0, Z) of the prior Block's output and adding its slice [2Z, 2Z + C) as a residual, no reparam entry in front -- is
recognised with and without z_feat_proj, and near misses are not."""
from types import SimpleNamespace

import pytest

Z, CW, CTX = 16, 32, 4


def _engine(det=True):
    from causal_gen_amd.engine import Engine

    eng = Engine.__new__(Engine)
    eng.tape, eng.lat_tail_det = [], det
    return eng


def _nt(c, rg=True):
    from causal_gen_amd.engine import NT

    return NT(0x10000, 2, 64, 64, c, 64 * 64 * c, 64 * c, c, 2, rg=rg)


def _layer(eng, feat=True, ks=1, loc=(0, Z), res=(2 * Z, 2 * Z + CW), loc_base=None, stochastic=False):
    """The tape entries of one layer in forward order (z_proj, [conv Block], z_feat_proj is inserted right behind z_proj)."""
    from causal_gen_amd.engine import ACT_NONE

    pout, h, pa = _nt(2 * Z + CW), _nt(CW), _nt(CTX, rg=False)
    p_loc = (loc_base if loc_base is not None else pout).chan(*loc)
    p_feat = pout.chan(*res)
    site_p = SimpleNamespace(ks=ks, co=CW, seg_rg=[True, False], name="z_proj")
    site_f = SimpleNamespace(ks=1, co=CW, seg_rg=[True, True], name="z_feat_proj")
    if stochastic:
        z = _nt(Z)
        eng.tape.append((eng._bw_reparam, (pout.chan(0, Z), pout.chan(Z, 2 * Z), pout.chan(0, Z), pout.chan(Z, 2 * Z), z, 0.0, None, None), 0))
        p_loc = z
    eng.tape.append((eng._bw_conv, (site_p, [p_loc, pa], ACT_NONE, _nt(CW), h, p_feat), 0))
    if feat:
        eng.tape.append((eng._bw_conv, (site_f, [p_loc, p_feat], ACT_NONE, _nt(CW), None, None), 0))
    return len(eng.tape) - 1


@pytest.mark.parametrize("feat", [True, False])
def test_the_deterministic_pattern_is_accepted(feat):
    eng = _engine()
    i = _layer(eng, feat)
    f, a, r = eng._latent_tail_at(i)
    assert r is None and a is eng.tape[i - 1 if feat else i][1] and (f is eng.tape[i][1] if feat else f is None)


def test_the_knob_turns_it_off():
    eng = _engine(det=False)
    assert eng._latent_tail_at(_layer(eng)) is None


@pytest.mark.parametrize("feat", [True, False])
@pytest.mark.parametrize("miss", ["other_base", "residual_slice", "ks3", "loc_offset"])
def test_near_misses_are_rejected(miss, feat):
    eng = _engine()
    kw = {"other_base": dict(loc_base=_nt(2 * Z + CW)),         # the first segment is a slice of another tensor
          "residual_slice": dict(res=(Z, Z + CW)),              # the residual is not [2Z, 2Z + C)
          "ks3": dict(ks=3),                                    # a 3x3 site
          "loc_offset": dict(loc=(Z, 2 * Z))}[miss]             # the first segment is not [0, Z)
    assert eng._latent_tail_at(_layer(eng, feat, **kw)) is None


def test_a_whole_tensor_as_first_segment_is_not_the_pattern():
    """A stochastic layer's z is a tensor of its own: without its reparam entry in front it is left to the separate launches."""
    eng = _engine()
    i = _layer(eng, stochastic=True)
    del eng.tape[i - 2]  # (the reparam entry)
    assert eng._latent_tail_at(i - 1) is None
