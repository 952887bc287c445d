"""Counterfactual evaluation without a GPU: argument validation before any launch, the metric tables of the four data sets, and
the f64 AUC reference of the GPU tests against sklearn.  (The record's layout against the header: tests/test_abi_mirror.py.)"""
import numpy as np
import pytest

import cf_eval_ref as R


def _var(**kw):
    from causal_gen_amd import _lib

    r = _lib.MetricVar()
    r.kind, r.transform, r.ncls = _lib.METRIC_BINARY, _lib.METRIC_SIGMOID, 1
    # fake device addresses: validation must reject before anything dereferences them
    r.pred, r.pred_stride, r.target, r.target_stride, r.acc, r.norm = 4096, 16, 8192, 1, 12288, 1.0
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_metric_accum_rejects_bad_arguments_before_any_launch():
    from causal_gen_amd import _lib

    lib = _lib.load()
    one = lambda r: (_lib.MetricVar * 1)(r)
    with pytest.raises(_lib.CgenError, match="null vars"):
        lib.metric_accum(None, 1, 4, None)
    with pytest.raises(_lib.CgenError, match="ncls 17 outside"):
        lib.metric_accum(one(_var(kind=_lib.METRIC_CATEGORICAL, transform=_lib.METRIC_SOFTMAX, ncls=17, pred_stride=32, target_stride=32)), 1, 4, None)
    with pytest.raises(_lib.CgenError, match="unknown kind 9"):
        lib.metric_accum(one(_var(kind=9)), 1, 4, None)
    with pytest.raises(_lib.CgenError, match="n -1 is negative"):
        lib.metric_accum(one(_var()), 1, -1, None)
    with pytest.raises(_lib.CgenError, match="unknown transform 5"):
        lib.metric_accum(one(_var(transform=5)), 1, 4, None)
    with pytest.raises(_lib.CgenError, match="transform 3 does not fit kind 0"):
        lib.metric_accum(one(_var(transform=_lib.METRIC_TANH)), 1, 4, None)
    with pytest.raises(_lib.CgenError, match="null pred, target or acc"):
        lib.metric_accum(one(_var(acc=None)), 1, 4, None)
    with pytest.raises(_lib.CgenError, match="pred_stride 3 < ncls 4"):
        lib.metric_accum(one(_var(kind=_lib.METRIC_CATEGORICAL, transform=_lib.METRIC_SOFTMAX, ncls=4, pred_stride=3, target_stride=4)), 1, 4, None)
    with pytest.raises(_lib.CgenError, match="must be given together"):
        lib.metric_accum(one(_var(scores=4096)), 1, 4, None)
    with pytest.raises(_lib.CgenError, match="nvars 9 outside"):
        lib.metric_accum(one(_var()), 9, 4, None)
    assert lib._raw_cgen_metric_accum(one(_var()), 1, 0, None) == 0  # an empty batch launches nothing


def test_rocauc_and_image_dist_reject_bad_arguments_before_any_launch():
    from causal_gen_amd import _lib

    lib = _lib.load()
    with pytest.raises(_lib.CgenError, match="null scores"):
        lib.rocauc(None, 4096, 4096, 10, 1, 1, 4096, 4096, None)
    with pytest.raises(_lib.CgenError, match="ncls 17 outside"):
        lib.rocauc(4096, 4096, 4096, 10, 17, 17, 4096, 4096, None)
    with pytest.raises(_lib.CgenError, match="stride 2 < ncls 3"):
        lib.rocauc(4096, 4096, 4096, 10, 3, 2, 4096, 4096, None)
    with pytest.raises(_lib.CgenError, match="n_rows_max"):
        lib.rocauc(4096, 4096, 4096, 1 << 31, 1, 1, 4096, 4096, None)
    with pytest.raises(_lib.CgenError, match="null a, b or ws"):
        lib.image_dist(2, 1024, 4096, None, None, 4096, None, None)
    with pytest.raises(_lib.CgenError, match="elems_per_image 0"):
        lib.image_dist(2, 0, 4096, 4096, None, 4096, None, None)
    assert lib._raw_cgen_image_dist(0, 1024, 4096, 4096, None, 4096, None, None) == 0


def test_metric_specs_tables():
    from causal_gen_amd import cf_eval
    from causal_gen_amd.dscm import _UKBB_MIN_MAX

    def keys(specs):
        return sorted(s.name + "_" + m for s in specs for m in s.metrics)

    uk = {s.name: s for s in cf_eval.metric_specs("ukbb192")}
    assert keys(uk.values()) == sorted(["sex_rocauc", "sex_acc", "mri_seq_rocauc", "mri_seq_acc", "age_mae", "brain_volume_mae",
                                        "ventricle_volume_mae"])
    assert uk["sex"].kind == "binary" and uk["sex"].transform == "sigmoid" and uk["mri_seq"].transform == "sigmoid"
    for k in ("age", "brain_volume", "ventricle_volume"):
        hi, lo = _UKBB_MIN_MAX[k]
        s = uk[k]
        assert s.kind == "continuous" and s.transform == "none"
        # [-1, 1] -> [min, max] on both sides: -1 -> min, +1 -> max
        assert abs(-s.pred_scale + s.pred_shift - lo) <= 1e-9 * hi and abs(s.pred_scale + s.pred_shift - hi) <= 1e-9 * hi
        assert (s.tgt_scale, s.tgt_shift) == (s.pred_scale, s.pred_shift)
        assert s.norm == (1000.0 if "volume" in k else 1.0)
    assert all(s.transform == "none" for s in cf_eval.metric_specs("ukbb192", raw=False))

    mm = {"thickness": (0.5, 7.5), "intensity": (60.0, 255.0)}
    mo = {s.name: s for s in cf_eval.metric_specs("morphomnist", mm)}
    assert keys(mo.values()) == ["digit_acc", "intensity_mae", "thickness_mae"]
    assert mo["digit"].kind == "categorical" and mo["digit"].ncls == 10
    assert mo["thickness"].transform == "tanh" and (mo["thickness"].pred_scale, mo["thickness"].pred_shift) == (3.5, 4.0)
    assert (mo["intensity"].tgt_scale, mo["intensity"].tgt_shift) == (97.5, 157.5)
    plain = {s.name: s for s in cf_eval.metric_specs("morphomnist")}
    assert (plain["thickness"].pred_scale, plain["thickness"].pred_shift) == (1.0, 0.0)

    cm = cf_eval.metric_specs("cmnist")
    assert keys(cm) == ["colour_acc", "digit_acc"] and all(s.ncls == 10 and s.kind == "categorical" for s in cm)

    mi = {s.name: s for s in cf_eval.metric_specs("mimic224")}
    assert keys(mi.values()) == sorted(["sex_rocauc", "sex_acc", "finding_rocauc", "finding_acc", "age_mae", "race_acc", "race_rocauc"])
    assert all(s.transform == "none" for s in mi.values())
    assert (mi["age"].pred_scale, mi["age"].pred_shift, mi["age"].tgt_scale, mi["age"].tgt_shift) == (50.0, 50.0, 50.0, 50.0)
    assert mi["race"].kind == "categorical" and mi["race"].ncls == 3
    with pytest.raises(ValueError):
        cf_eval.metric_specs("celeba")


def test_counting_form_of_the_auc_reference_equals_the_definition():
    g = np.random.default_rng(0)
    for n, levels in ((2, None), (65, 4), (300, None), (301, 3)):
        s = g.standard_normal(n)
        if levels:
            s = np.floor(g.random(n) * levels) / levels
        lab = (g.random(n) < 0.4).astype(np.float64)
        lab[0], lab[-1] = 1.0, 0.0
        assert R.auc_pairs(s, lab) == R.auc_pairs_brute(s, lab)
    assert np.isnan(R.auc_pairs(np.arange(5.0), np.ones(5))) and np.isnan(R.auc_pairs(np.arange(5.0), np.zeros(5)))
    assert R.auc_pairs(np.ones(9), np.arange(9) % 2) == 0.5


def test_auc_reference_equals_sklearn_with_heavy_ties():
    skm = pytest.importorskip("sklearn.metrics")
    g = np.random.default_rng(1)
    n = 2000
    lab = (g.random(n) < 0.3).astype(np.float64)
    s = np.floor((g.random(n) * 0.7 + lab * 0.3) * 4) / 4  # 4 levels
    assert len(np.unique(s)) == 4
    want = skm.roc_auc_score(lab, s, average="macro")
    assert abs(R.auc_pairs(s, lab) - want) <= 1e-12
    assert abs(R.binary_metrics(s, lab, transform="none")["rocauc"] - want) <= 1e-12


def test_auc_reference_equals_sklearn_three_class_ovr_macro():
    skm = pytest.importorskip("sklearn.metrics")
    g = np.random.default_rng(2)
    n = 1500
    k = g.integers(0, 3, n)
    logits = g.standard_normal((n, 3)) + 1.2 * np.eye(3)[k]
    p = R.softmax(logits)
    want = skm.roc_auc_score(np.eye(3)[k], p, multi_class="ovr", average="macro")
    assert abs(R.auc_ovr_macro(p, np.eye(3)[k]) - want) <= 1e-12
    assert abs(R.categorical_metrics(logits, np.eye(3)[k], 3)["rocauc"] - want) <= 1e-12
