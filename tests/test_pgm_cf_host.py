"""The host side of the device counterfactual, without a GPU: the preprocess records of the four data sets' ``parents_x`` against
hand-written expectations, the touched-set rule against ``pgm.counterfactual`` in f64 (what the kernel copies is what the
reference leaves at the observation; what it recomputes is exactly the descendants of the intervened variable), and the ``u=``
argument of the two Gumbel-max abductions."""
from types import SimpleNamespace

import pytest
import torch

import pgm_cases as PC


def test_preprocess_records_of_the_four_parents_x():
    from causal_gen_amd import _lib
    from causal_gen_amd import pgm_cf as CF
    from causal_gen_amd.pgm_train import default_columns

    COPY, LOG = _lib.PGM_PRE_COPY, _lib.PGM_PRE_LOGSTD
    f32 = lambda v: torch.tensor(v, dtype=torch.float32).item()

    def recs(kind, parents_x, dataset):
        m = PC.make_pgm(kind)
        cols, ncol = default_columns(m)
        return CF.pre_records(m, SimpleNamespace(parents_x=parents_x, dataset=dataset), cols, ncol)

    # ukbb: table columns sex 0, mri_seq 1, age 2, brain_volume 3, ventricle_volume 4; the constants are dscm.ukbb_preprocess's
    got = recs("flow", ["mri_seq", "brain_volume", "ventricle_volume", "sex"], "ukbb192")
    assert got == [(1, 1, COPY, 0.0, 0.0, 0.0, 1.0),
                   (3, 1, LOG, 1629520.0, 841919.0, 13.965583801269531, 0.09537758678197861),
                   (4, 1, LOG, 157075.0, 7613.27001953125, 10.345998764038086, 0.43127763271331787),
                   (0, 1, COPY, 0.0, 0.0, 0.0, 1.0)]
    for r in got:  # every constant is an f32 value: the record's floats carry it exactly
        assert all(f32(v) == v for v in r[3:])
    got = recs("flow", ["age"], "ukbb64")
    assert got == [(2, 1, LOG, 73.0, 44.0, 4.112339973449707, 0.11769197136163712)]
    # morphomnist: thickness 0, intensity 1, digit 2..11 -- nothing is transformed
    assert recs("morpho", ["thickness", "intensity", "digit"], "morphomnist") == [(0, 1, COPY, 0.0, 0.0, 0.0, 1.0), (1, 1, COPY, 0.0, 0.0, 0.0, 1.0),
                                                                                 (2, 10, COPY, 0.0, 0.0, 0.0, 1.0)]
    # cmnist: digit 0..9, colour 10..19
    assert recs("colour", ["digit", "colour"], "cmnist") == [(0, 10, COPY, 0.0, 0.0, 0.0, 1.0), (10, 10, COPY, 0.0, 0.0, 0.0, 1.0)]
    # mimic: race 0..2, sex 3, finding 4, age 5
    assert recs("chest", ["age", "race", "sex", "finding"], "mimic") == [(5, 1, COPY, 0.0, 0.0, 0.0, 1.0), (0, 3, COPY, 0.0, 0.0, 0.0, 1.0),
                                                                         (3, 1, COPY, 0.0, 0.0, 0.0, 1.0), (4, 1, COPY, 0.0, 0.0, 0.0, 1.0)]
    with pytest.raises(ValueError, match="no column was named for parent 'weight'"):
        recs("flow", ["weight"], "ukbb192")
    with pytest.raises(ValueError, match="9 entries"):
        recs("flow", ["age"] * 9, "ukbb192")
    with pytest.raises(ValueError, match="0 entries"):
        recs("flow", [], "ukbb192")


def _descendants(m, var):
    """`var` and everything reachable from it along context -> variable edges (its own closure, not the helper's loop)."""
    edges = [(c, mech.var) for mech in m.mechanisms() for c in mech.ctx]
    seen, frontier = {var}, [var]
    while frontier:
        v = frontier.pop()
        for a, b in edges:
            if a == v and b not in seen:
                seen.add(b)
                frontier.append(b)
    return seen


@pytest.mark.parametrize("kind", PC.KINDS)
def test_the_copy_rule_is_the_reference_semantics(kind):
    """For every single-variable intervention: the variables the kernel copies are left at the observation by the f64 host
    (within 1e-12: it recomputes f(f^-1(obs))), and the variables it treats as touched are exactly the descendants."""
    from causal_gen_amd import pgm_cf as CF

    m = PC.make_pgm(kind, seed=41)
    m64 = PC.to64(m)
    obs = PC.cast(PC.draw(m, 97, seed=12), torch.float64)
    perm = torch.randperm(97, generator=torch.Generator().manual_seed(7))
    for var in m.variables:
        do = {var: obs[var][perm]}
        t = CF.touched(m, [var])
        assert set(t) == _descendants(m, var), (var, t)
        assert t == [mech.var for mech in m.mechanisms() if mech.var in t]  # in mechanism order
        with torch.no_grad():
            cf = m64.counterfactual(obs, do)
        for k in m.variables:
            if k not in t:
                err = (cf[k] - obs[k]).abs().max().item()
                assert err <= 1e-12, (var, k, err)
        assert torch.equal(cf[var], do[var])
    assert CF.touched(m, []) == []
    assert CF.touched(m, list(m.variables)) == [mech.var for mech in m.mechanisms()]
    if kind == "flow":
        assert CF.touched(m, ["sex"]) == ["sex", "brain_volume", "ventricle_volume"] and CF.touched(m, ["mri_seq"]) == ["mri_seq"]
        assert CF.touched(m, ["age", "sex"]) == ["sex", "age", "brain_volume", "ventricle_volume"]
    if kind == "chest":  # flow_pgm.py:96-105: finding keeps its observed value unless age or finding is intervened on
        assert CF.touched(m, ["age"]) == ["age", "finding"] and CF.touched(m, ["sex"]) == ["sex"] and CF.touched(m, ["race"]) == ["race"]


@pytest.mark.parametrize("exact", (False, True))
def test_gumbel_abduction_takes_its_uniforms(exact):
    from causal_gen_amd import pgm as P

    fn = P.gumbel_max_abduct_exact if exact else P.gumbel_max_abduct
    g = torch.Generator().manual_seed(5)
    logits = torch.log_softmax(torch.randn(50, 3, generator=g, dtype=torch.float64), -1)
    k = torch.randint(0, 3, (50, 1), generator=g).double()
    # the default draws as before: the same generator state gives the same noise as passing those uniforms
    a = fn(k, logits, torch.Generator().manual_seed(9))
    u = torch.rand(logits.shape, dtype=logits.dtype, generator=torch.Generator().manual_seed(9))
    b = fn(k, logits, u=u)
    assert torch.equal(a, b) and torch.equal(b, fn(k, logits, u=u))
    assert not torch.equal(b, fn(k, logits, u=u.flip(0)))
    if exact:
        assert torch.equal(P.gumbel_max_forward(b, logits), k.long())
