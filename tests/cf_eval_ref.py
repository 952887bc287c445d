"""f64 numpy restatement of the evaluation numbers for the cf_eval tests: the per-variable metrics of get_metrics / eval_epoch
(train_cf.py:63-108, train_pgm.py:196-249), the Mann-Whitney pair form of the ROC-AUC, and the per-image distances.  Every
function takes what the device takes (raw head outputs or predictions, targets) as arrays and works in float64."""
import numpy as np


def _2d(a):
    a = np.asarray(a)
    return a.reshape(a.shape[0], -1)


def finite_rows(pred, target, ncls_pred=1, ncls_target=1):
    """Rows whose first ncls prediction columns and target columns are all finite (the others are skipped)."""
    p, t = _2d(pred)[:, :ncls_pred], _2d(target)[:, :ncls_target]
    return np.isfinite(p).all(1) & np.isfinite(t).all(1)


def sigmoid(o):
    return 1.0 / (1.0 + np.exp(-np.asarray(o, dtype=np.float64)))


def softmax(o):
    o = np.asarray(o, dtype=np.float64)
    e = np.exp(o - o.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def auc_pairs(scores, labels):
    """(#{s+ > s-} + 0.5 #{s+ == s-}) / (n+ n-) over all positive / negative pairs; NaN when a class is absent."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    pos_mask = np.asarray(labels).reshape(-1) > 0.5
    pos, neg = s[pos_mask], s[~pos_mask]
    if pos.size == 0 or neg.size == 0:
        return float("nan")
    neg_sorted = np.sort(neg)
    less = np.searchsorted(neg_sorted, pos, side="left").astype(np.int64)      # negatives strictly below each positive
    less_eq = np.searchsorted(neg_sorted, pos, side="right").astype(np.int64)  # ... below or equal
    gt, eq = int(less.sum()), int((less_eq - less).sum())
    return (gt + 0.5 * eq) / (float(pos.size) * float(neg.size))


def auc_pairs_brute(scores, labels):
    """The same by the definition, O(n^2): the check of the counting form above."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    pos_mask = np.asarray(labels).reshape(-1) > 0.5
    pos, neg = s[pos_mask], s[~pos_mask]
    if pos.size == 0 or neg.size == 0:
        return float("nan")
    gt = int((pos[:, None] > neg[None, :]).sum())
    eq = int((pos[:, None] == neg[None, :]).sum())
    return (gt + 0.5 * eq) / (float(pos.size) * float(neg.size))


def auc_ovr_macro(scores, onehot):
    """One-vs-rest macro AUC: the mean of the per-column binary AUCs (roc_auc_score(multi_class="ovr", average="macro"))."""
    s, l = _2d(scores), _2d(onehot)
    return float(np.mean([auc_pairs(s[:, c], l[:, c]) for c in range(s.shape[1])]))


def binary_metrics(pred, target, transform="sigmoid", capacity=None):
    """{"n", "n_skipped", "correct", "acc", "rocauc", "scores", "labels"}: pred raw logits (transform "sigmoid") or probabilities
    ("none"); round(sigmoid(o)) == t is (o > 0) == t, round(p) == t is (p > 0.5) == t.  The AUC uses the first `capacity` kept rows."""
    p, t = _2d(pred)[:, 0].astype(np.float64), _2d(target)[:, 0].astype(np.float64)
    keep = np.isfinite(p) & np.isfinite(t)
    p, t = p[keep], t[keep]
    lab = t > 0.5
    hit = (p > 0.0) if transform == "sigmoid" else (p > 0.5)
    score = sigmoid(p) if transform == "sigmoid" else p
    cap = len(p) if capacity is None else min(capacity, len(p))
    n = len(p)
    return {"n": n, "n_skipped": int((~keep).sum()), "correct": int((hit == lab).sum()), "acc": float((hit == lab).sum()) / n if n else float("nan"),
            "rocauc": auc_pairs(score[:cap], lab[:cap]), "scores": score[:cap], "labels": lab[:cap].astype(np.float64),
            "n_overflow": n - cap}


def categorical_metrics(pred, target, ncls, transform="softmax", capacity=None):
    p, t = _2d(pred)[:, :ncls].astype(np.float64), _2d(target)[:, :ncls].astype(np.float64)
    keep = np.isfinite(p).all(1) & np.isfinite(t).all(1)
    p, t = p[keep], t[keep]
    ap, at = p.argmax(1), t.argmax(1)  # numpy's argmax takes the first maximum
    n = len(p)
    cap = n if capacity is None else min(capacity, n)
    score = softmax(p) if transform == "softmax" else p
    onehot = np.eye(ncls)[at]
    return {"n": n, "n_skipped": int((~keep).sum()), "correct": int((ap == at).sum()), "acc": float((ap == at).sum()) / n if n else float("nan"),
            "rocauc": auc_ovr_macro(score[:cap], onehot[:cap]) if cap else float("nan"), "scores": score[:cap], "labels": onehot[:cap],
            "n_overflow": n - cap}


def continuous_metrics(pred, target, transform="none", pred_scale=1.0, pred_shift=0.0, tgt_scale=1.0, tgt_shift=0.0, norm=1.0):
    """mean |(t * tgt_scale + tgt_shift) - (f(o) * pred_scale + pred_shift)| / norm with the constants rounded to f32 first, as the
    record carries them."""
    f32 = lambda v: float(np.float32(v))
    p, t = _2d(pred)[:, 0].astype(np.float64), _2d(target)[:, 0].astype(np.float64)
    keep = np.isfinite(p) & np.isfinite(t)
    p, t = p[keep], t[keep]
    f = np.tanh(p) if transform == "tanh" else p
    err = np.abs((t * f32(tgt_scale) + f32(tgt_shift)) - (f * f32(pred_scale) + f32(pred_shift))) / f32(norm)
    n = len(p)
    return {"n": n, "n_skipped": int((~keep).sum()), "abs_err": float(err.sum()), "mae": float(err.sum()) / n if n else float("nan")}


def spec_metrics(spec, pred, target, capacity=None):
    """The result keys of one cf_eval.MetricSpec on (pred, target): {"<name>_acc" / "_rocauc" / "_mae", "n", "n_skipped", "n_overflow"}."""
    if spec.kind == "binary":
        m = binary_metrics(pred, target, spec.transform, capacity)
    elif spec.kind == "categorical":
        m = categorical_metrics(pred, target, spec.ncls, spec.transform, capacity)
    else:
        m = continuous_metrics(pred, target, spec.transform, spec.pred_scale, spec.pred_shift, spec.tgt_scale, spec.tgt_shift, spec.norm)
    out = {"n": m["n"], "n_skipped": m["n_skipped"], "n_overflow": m.get("n_overflow", 0) if "rocauc" in spec.metrics else 0}
    for k in spec.metrics:
        out[spec.name + "_" + k] = m[k]
    return out


def image_dist(a, b):
    """[B, 2] f64: per-image mean |a - b| and mean (a - b)^2."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = (a - b).reshape(a.shape[0], -1)
    return np.stack([np.abs(d).mean(1), (d * d).mean(1)], 1)
