"""Counterfactual evaluation on the device -- the evaluation half of ``train_cf.py`` / ``train_pgm.py``.

The reference collects every batch of predictions on the host and calls sklearn: ``get_metrics`` (train_cf.py:63-108) over what the
``else`` branch of ``cf_epoch`` gathers (train_cf.py:181-189), and ``eval_epoch`` (train_pgm.py:175-249) on factual images.  Here
the numbers are accumulated where the predictions are: ``MetricAccumulator`` feeds the predictors' raw head outputs to
``cgen_metric_accum`` in place (accuracy, mean absolute error, the score rows of the AUC), ``compute()`` runs the exact pair-count
ROC-AUC (``cgen_rocauc``) and reads everything back once.  ``CfEvaluator`` adds the three soundness measures of a deep SCM:
effectiveness (do the anticausal predictors find the intervened value in the counterfactual?), composition (how far does a null
intervention move the image?) and reversibility (how far does an intervention followed by its undo move it?); the last two are
image-side loops over ``dscm.counterfactual`` measured by ``cgen_image_dist``.  Every number is bit-identical from run to run.
"""
from dataclasses import dataclass, replace
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from . import _lib
from .dscm import _UKBB_MIN_MAX, cf_pixels, counterfactual, vae_preprocess

_KINDS = {"binary": _lib.METRIC_BINARY, "categorical": _lib.METRIC_CATEGORICAL, "continuous": _lib.METRIC_CONTINUOUS}
_TRANSFORMS = {"none": _lib.METRIC_NONE, "sigmoid": _lib.METRIC_SIGMOID, "softmax": _lib.METRIC_SOFTMAX, "tanh": _lib.METRIC_TANH}


@dataclass(frozen=True)
class MetricSpec:
    """One variable of the metric table.  ``transform`` is what ``predict()`` applies to the raw head output ("none" when the
    predictions handed in are already probabilities / values); ``metrics`` is a subset of ("rocauc", "acc") or ("mae",).
    Continuous: ``|(t * tgt_scale + tgt_shift) - (f(o) * pred_scale + pred_shift)| / norm``."""
    name: str
    kind: str
    ncls: int = 1
    transform: str = "none"
    metrics: Tuple[str, ...] = ()
    pred_scale: float = 1.0
    pred_shift: float = 0.0
    tgt_scale: float = 1.0
    tgt_shift: float = 0.0
    norm: float = 1.0


def _unit_range(lo: float, hi: float) -> Tuple[float, float]:
    """(scale, shift) of [-1, 1] -> [lo, hi]: ((v + 1) / 2) * (hi - lo) + lo."""
    return (hi - lo) / 2.0, (hi + lo) / 2.0


def metric_specs(dataset: str, min_max: Optional[Dict[str, Sequence[float]]] = None, raw: bool = True) -> List[MetricSpec]:
    """The per-variable table of ``get_metrics`` (train_cf.py:63-108) and ``eval_epoch`` (train_pgm.py:196-249).

    ukbb: ``sex`` and ``mri_seq`` ROC-AUC and accuracy; ``age``, ``brain_volume`` and ``ventricle_volume`` mean absolute error in
    original units (both sides taken from the [-1, 1] normalisation back to [min, max]; volumes in ml, i.e. / 1000).
    morphomnist: digit accuracy; thickness and intensity MAE, both sides unnormalised with ``min_max[k] = (min, max)`` (the data
    set's; without it the error stays on the [-1, 1] scale).  cmnist: digit and colour accuracy.  mimic (the table for predictions that are
    probabilities already -- ``ChestPredictor.predict()``'s or a reference predictor's -- so every transform is "none";
    ``chest_metric_specs()`` is the table for ``predictor_resnet.ChestPredictor``'s raw head outputs): sex and finding
    ROC-AUC and accuracy, age MAE with (v + 1) * 50 on both sides, race accuracy and one-vs-rest macro ROC-AUC.
    ``raw=True``: the predictions are raw head outputs (``predictor.raw_outputs``); ``raw=False``: they are ``predict()``'s."""
    ds = dataset or ""
    tr = (lambda t: t) if raw else (lambda t: "none")
    if "ukbb" in ds:
        out = [MetricSpec(k, "binary", 1, tr("sigmoid"), ("rocauc", "acc")) for k in ("sex", "mri_seq")]
        for k in ("age", "brain_volume", "ventricle_volume"):
            hi, lo = _UKBB_MIN_MAX[k]
            sc, sh = _unit_range(lo, hi)
            out.append(MetricSpec(k, "continuous", 1, "none", ("mae",), sc, sh, sc, sh, 1000.0 if "volume" in k else 1.0))
        return out
    if "morphomnist" in ds:
        out = []
        for k in ("thickness", "intensity"):
            sc, sh = _unit_range(float(min_max[k][0]), float(min_max[k][1])) if min_max is not None else (1.0, 0.0)
            out.append(MetricSpec(k, "continuous", 1, tr("tanh"), ("mae",), sc, sh, sc, sh, 1.0))
        return out + [MetricSpec("digit", "categorical", 10, tr("softmax"), ("acc",))]
    if "cmnist" in ds:
        return [MetricSpec(k, "categorical", 10, tr("softmax"), ("acc",)) for k in ("digit", "colour")]
    if "mimic" in ds:
        return [MetricSpec("sex", "binary", 1, "none", ("rocauc", "acc")), MetricSpec("finding", "binary", 1, "none", ("rocauc", "acc")),
                MetricSpec("age", "continuous", 1, "none", ("mae",), 50.0, 50.0, 50.0, 50.0, 1.0),
                MetricSpec("race", "categorical", 3, "none", ("acc", "rocauc"))]
    raise ValueError(f"no metric table for dataset {dataset!r}")


def chest_metric_specs(raw: bool = True) -> List[MetricSpec]:
    """The mimic table of ``metric_specs`` with the transforms ``predictor_resnet.ChestPredictor``'s raw head outputs need:
    sigmoid for sex and finding, softmax for race, none for age (its (v + 1) * 50 scaling stays) -- so that
    ``MetricAccumulator(chest_metric_specs()).update_from(ChestPredictor, ...)`` works in place like the other data sets.
    ``raw=False``: ``metric_specs("mimic")`` itself (for ``predict()``'s probabilities)."""
    tr = {"sex": "sigmoid", "finding": "sigmoid", "race": "softmax", "age": "none"}
    return [replace(s, transform=tr[s.name]) if raw else s for s in metric_specs("mimic")]


def _rows(v: Tensor, n: Optional[int], device, what: str) -> Tensor:
    """[n, k] f32 rows on `device` with unit column stride; a row-strided view (e.g. one head of the predictor's output buffer)
    is taken as it is."""
    if v.dim() == 1:
        v = v[:, None]
    if v.dim() != 2:
        v = v.reshape(v.shape[0], -1)
    v = v.detach()
    if v.dtype != torch.float32 or v.device != device:
        v = v.to(device=device, dtype=torch.float32)
    in_place = (v.shape[1] == 1 or v.stride(1) == 1) and (v.shape[0] == 1 or v.stride(0) >= v.shape[1])
    if not in_place:
        v = v.contiguous()
    if n is not None and v.shape[0] != n:
        raise ValueError(f"{what}: {v.shape[0]} rows, the other variables have {n}")
    return v


class MetricAccumulator:
    """Running metrics of ``specs`` over batches.  ``update`` is one ``cgen_metric_accum`` launch and never synchronises;
    ``compute`` runs one ``cgen_rocauc`` per AUC variable and then reads the device ONCE.  At most ``capacity`` rows per variable
    take part in the AUC (later rows are counted in ``n_overflow`` and still count for accuracy)."""

    def __init__(self, specs: Sequence[MetricSpec], capacity: int = 65536, device="cuda"):
        self.lib = _lib.require_gpu()
        self.specs = list(specs)
        self.capacity = int(capacity)
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if not 0 <= self.capacity < 2 ** 31:
            raise ValueError(f"capacity {capacity} outside 0..2^31-1")
        nv = len(self.specs)
        dev = self.device
        self.acc = torch.zeros(nv, _lib.METRIC_ACC, dtype=torch.float64, device=dev)
        self.auc = torch.full((nv, _lib.PRED_MAX_OUT), float("nan"), dtype=torch.float64, device=dev)
        self.row_count = torch.zeros(nv, dtype=torch.int64, device=dev)
        self._ws = torch.zeros(4 * _lib.PRED_MAX_OUT, dtype=torch.int64, device=dev)
        self.scores: Dict[str, Tensor] = {}
        self.labels: Dict[str, Tensor] = {}
        for s in self.specs:
            if s.kind not in _KINDS or s.transform not in _TRANSFORMS:
                raise ValueError(f"{s.name}: unknown kind {s.kind!r} or transform {s.transform!r}")
            if "rocauc" in s.metrics:
                if s.kind == "continuous":
                    raise ValueError(f"{s.name}: a continuous variable has no ROC-AUC")
                self.scores[s.name] = torch.zeros(self.capacity, s.ncls, device=dev)
                self.labels[s.name] = torch.zeros(self.capacity, s.ncls, device=dev)

    def reset(self):
        self.acc.zero_()
        self.row_count.zero_()
        self.auc.fill_(float("nan"))

    def update(self, preds: Dict[str, Tensor], targets: Dict[str, Tensor]):
        """One batch: ``preds[name]`` raw head outputs (or any [B, k] tensor; the first ``ncls`` columns are read), ``targets[name]``
        [B, 1] / one-hot [B, ncls].  Variables of the table that ``preds`` lacks are left alone."""
        recs, keep, n = [], [], None
        for i, s in enumerate(self.specs):
            if s.name not in preds:
                continue
            p = _rows(preds[s.name], n, self.device, s.name)
            n = p.shape[0]
            t = _rows(targets[s.name], n, self.device, s.name + " target")
            if p.shape[1] < s.ncls or (s.kind == "categorical" and t.shape[1] < s.ncls):
                raise ValueError(f"{s.name}: needs {s.ncls} columns, got predictions {tuple(p.shape)} and targets {tuple(t.shape)}")
            r = _lib.MetricVar()
            r.kind, r.transform, r.ncls = _KINDS[s.kind], _TRANSFORMS[s.transform], s.ncls
            r.pred, r.pred_stride = p.data_ptr(), max(p.stride(0), s.ncls) if n > 1 else max(p.shape[1], s.ncls)
            r.target, r.target_stride = t.data_ptr(), max(t.stride(0), 1) if n > 1 else t.shape[1]
            r.pred_scale, r.pred_shift, r.tgt_scale, r.tgt_shift, r.norm = s.pred_scale, s.pred_shift, s.tgt_scale, s.tgt_shift, s.norm
            r.acc = self.acc[i].data_ptr()
            if s.name in self.scores:
                r.scores, r.labels = self.scores[s.name].data_ptr(), self.labels[s.name].data_ptr()
                r.capacity, r.row_count = self.capacity, self.row_count[i:].data_ptr()
            recs.append(r)
            keep += [p, t]
        if not recs or n == 0:
            return
        stream = torch.cuda.current_stream(self.device).cuda_stream
        for lo in range(0, len(recs), _lib.METRIC_MAX_VARS):
            part = recs[lo:lo + _lib.METRIC_MAX_VARS]
            self.lib.metric_accum((_lib.MetricVar * len(part))(*part), len(part), n, stream)

    def update_from(self, predictor, targets: Optional[Dict[str, Tensor]] = None, **obs):
        """Run the predictor's forward on ``obs`` (``x`` and the context variables) and feed its raw outputs straight to the
        metric kernel -- no torch sigmoid / softmax pass in between.  ``targets`` default to ``obs`` itself (``eval_epoch``)."""
        self.update(predictor.raw_outputs(**obs), obs if targets is None else targets)

    def compute(self) -> Dict[str, object]:
        """{``<var>_rocauc`` / ``<var>_acc`` / ``<var>_mae``: float, "n" / "n_skipped" / "n_overflow": {var: int}} -- the keys of
        ``get_metrics``; a categorical ROC-AUC is the one-vs-rest macro mean over the columns (train_cf.py:100-105)."""
        stream = torch.cuda.current_stream(self.device).cuda_stream
        # (the grid is sized by the capacity, not by a host-side row count: updates replayed from a captured graph append rows
        # the host never saw; workgroups past the device-side count leave at once)
        for i, s in enumerate(self.specs):
            if s.name in self.scores:
                self.lib.rocauc(self.scores[s.name].data_ptr(), self.labels[s.name].data_ptr(), self.row_count[i:].data_ptr(),
                                self.capacity, s.ncls, s.ncls, self.auc[i].data_ptr(), self._ws.data_ptr(), stream)
        host = torch.cat([self.acc.reshape(-1), self.auc.reshape(-1)]).cpu()  # the one host read
        nv = len(self.specs)
        acc = host[:nv * _lib.METRIC_ACC].reshape(nv, _lib.METRIC_ACC)
        auc = host[nv * _lib.METRIC_ACC:].reshape(nv, _lib.PRED_MAX_OUT)
        out: Dict[str, object] = {"n": {}, "n_skipped": {}, "n_overflow": {}}
        for i, s in enumerate(self.specs):
            cnt = float(acc[i, _lib.METRIC_N])
            out["n"][s.name] = int(cnt)
            out["n_skipped"][s.name] = int(acc[i, _lib.METRIC_SKIPPED])
            out["n_overflow"][s.name] = int(acc[i, _lib.METRIC_OVERFLOW])
            nan = float("nan")
            for m in s.metrics:
                if m == "acc":
                    out[s.name + "_acc"] = float(acc[i, _lib.METRIC_CORRECT]) / cnt if cnt else nan
                elif m == "mae":
                    out[s.name + "_mae"] = float(acc[i, _lib.METRIC_ABS_ERR]) / cnt if cnt else nan
                elif m == "rocauc":
                    out[s.name + "_rocauc"] = float(auc[i, :s.ncls].mean())
        return out


def image_distance(a: Tensor, b: Tensor, acc: Optional[Tensor] = None) -> Tensor:
    """Per-image distances of two image batches of one shape: [B, 2] f32 = (mean |a - b|, mean (a - b)^2), formed in f64
    (``cgen_image_dist``).  ``acc`` (f64 [3], optional) gets (sum of the L1s, sum of the L2s, B) ADDED in a fixed order."""
    lib = _lib.require_gpu()
    if a.shape != b.shape or a.dim() < 2:
        raise ValueError(f"image_distance: shapes {tuple(a.shape)} and {tuple(b.shape)}")
    dev = a.device if a.is_cuda else torch.device("cuda", torch.cuda.current_device())
    ts = []
    for t in (a, b):
        t = t.detach().to(device=dev, dtype=torch.float32)
        ts.append(t if t.is_contiguous() else t.contiguous())
    n = a.shape[0]
    out = torch.empty(n, 2, device=dev)
    ws = torch.empty(n, 2, dtype=torch.float64, device=dev)
    if acc is not None and (acc.dtype != torch.float64 or acc.numel() < 3 or acc.device != dev or not acc.is_contiguous()):
        raise ValueError("image_distance: acc must be a contiguous f64 tensor of 3 on the images' device")
    if n:
        lib.image_dist(n, ts[0].numel() // n, ts[0].data_ptr(), ts[1].data_ptr(), out.data_ptr(), ws.data_ptr(),
                       acc.data_ptr() if acc is not None else None, torch.cuda.current_stream(dev).cuda_stream)
    return out


def _do_name(do: Dict[str, Tensor]) -> str:
    return "do(" + ",".join(do.keys()) + ")" if do else "null"


class CfEvaluator:
    """Effectiveness, composition and reversibility of a deep SCM (``vae`` + ``pgm`` + anticausal ``predictor``) over batches.

    ``effectiveness`` is the evaluation loop of train_cf.py:489-497 (``cf_epoch(split="valid")`` once per intervened variable)
    for one batch and a list of interventions.  The ONE intended difference from calling ``DSCM.forward`` K times: the batch is
    abducted once (``abduct_with_reconstruction``) and ``forward_latents`` + ``cf_pixels`` are replayed once per intervention, so
    the K counterfactuals share their exogenous noise and cost one abduction instead of K.  With ``vae.cond_prior`` the latents
    are unwrapped as ``dscm.counterfactual`` does.  Works with either ``compute_dtype`` of the HVAE."""

    def __init__(self, vae, pgm, predictor, args, capacity: int = 65536, specs: Optional[Sequence[MetricSpec]] = None,
                 min_max=None, t_abduct: float = 1.0):
        self.vae, self.pgm, self.predictor, self.args = vae, pgm, predictor, args
        self.capacity, self.t_abduct = capacity, t_abduct
        self.specs = list(specs) if specs is not None else metric_specs(getattr(args, "dataset", ""), min_max)
        self.metrics: Dict[str, MetricAccumulator] = {}
        self.dist: Dict[Tuple[str, int], Tensor] = {}

    def reset(self):
        self.metrics, self.dist = {}, {}

    def _pre(self, pa: Dict[str, Tensor]) -> Tensor:
        return vae_preprocess(self.args, {k: v.clone() for k, v in pa.items()})

    def _dist(self, key, a, b) -> Tensor:
        acc = self.dist.get(key)
        if acc is None:
            acc = self.dist[key] = torch.zeros(3, dtype=torch.float64, device=a.device)
        return image_distance(a, b, acc)

    @torch.no_grad()
    def effectiveness(self, obs: Dict[str, Tensor], interventions: Union[Sequence[Dict[str, Tensor]], Dict[str, Dict[str, Tensor]]],
                      return_images: bool = False):
        """Accumulate the predictors' metrics on the counterfactuals of one batch under each intervention (a list of ``do``
        dicts, named "do(<variables>)", or a {name: do} dict).  The targets are the counterfactual parents, with the intervened
        value for the intervened variable (train_cf.py:186-189).  Returns {name: cf_x} with ``return_images``."""
        named = interventions if isinstance(interventions, dict) else {_do_name(do): do for do in interventions}
        if not isinstance(interventions, dict) and len(named) != len(interventions):
            raise ValueError("two interventions on the same variables: pass a {name: do} dict to tell them apart")
        vae = self.vae
        pa = {k: v for k, v in obs.items() if k != "x"}
        x = obs["x"].cuda().float()
        zs, (rec_loc, rec_scale) = vae.abduct_with_reconstruction(x, self._pre(pa), t=self.t_abduct)
        if vae.cond_prior:
            zs = [z["z"] for z in zs]
        images = {}
        for name, do in named.items():
            cf_pa = self.pgm.counterfactual(obs=pa, intervention=do, num_particles=1)
            cf_loc, cf_scale = vae.forward_latents(zs, self._pre(cf_pa))
            cf_x = cf_pixels(x, rec_loc, rec_scale, cf_loc, cf_scale)
            targets = {k: (do[k] if k in do else v) for k, v in cf_pa.items()}
            acc = self.metrics.get(name)
            if acc is None:
                acc = self.metrics[name] = MetricAccumulator(self.specs, self.capacity, cf_x.device)
            acc.update_from(self.predictor, targets=targets, x=cf_x, **cf_pa)
            if return_images:
                images[name] = cf_x
        return images if return_images else None

    @torch.no_grad()
    def composition(self, obs: Dict[str, Tensor], cycles: int = 1) -> List[Tensor]:
        """Repeat the null intervention ``cycles`` times (each a fresh abduction of the previous result) and measure the distance
        to the original after every cycle.  Returns the per-image [B, 2] distances, one tensor per cycle."""
        pa = self._pre({k: v for k, v in obs.items() if k != "x"})
        x0 = obs["x"].cuda().float()
        xi, out = x0, []
        for c in range(1, cycles + 1):
            xi = counterfactual(self.vae, xi, pa, pa, t_abduct=self.t_abduct)
            out.append(self._dist(("composition", c), x0, xi))
        return out

    @torch.no_grad()
    def reversibility(self, obs: Dict[str, Tensor], do: Dict[str, Tensor], cycles: int = 1) -> List[Tensor]:
        """Intervene, undo with ``pgm.counterfactual(obs=cf_pa, intervention={k: obs[k]})``, measure the distance to the original;
        ``cycles`` round trips, every hop a fresh abduction of its own input.  Returns the per-image distances per cycle."""
        pa = {k: v for k, v in obs.items() if k != "x"}
        x0 = obs["x"].cuda().float()
        xi, out = x0, []
        for c in range(1, cycles + 1):
            cf_pa = self.pgm.counterfactual(obs=pa, intervention=do, num_particles=1)
            there = counterfactual(self.vae, xi, self._pre(pa), self._pre(cf_pa), t_abduct=self.t_abduct)
            back_pa = self.pgm.counterfactual(obs=cf_pa, intervention={k: pa[k] for k in do}, num_particles=1)
            xi = counterfactual(self.vae, there, self._pre(cf_pa), self._pre(back_pa), t_abduct=self.t_abduct)
            pa = back_pa
            out.append(self._dist(("reversibility", c), x0, xi))
        return out

    def results(self) -> Dict[str, Dict]:
        """{"effectiveness": {intervention: metrics}, "composition" / "reversibility": {cycle: {"l1", "l2", "l1_grey", "n"}}}.
        Distances are on the images' [-1, 1] scale; ``l1_grey`` is the L1 in 8-bit grey levels (x 127.5)."""
        out: Dict[str, Dict] = {"effectiveness": {k: m.compute() for k, m in self.metrics.items()}, "composition": {}, "reversibility": {}}
        if self.dist:
            keys = list(self.dist)
            host = torch.stack([self.dist[k] for k in keys]).cpu()
            for (kind, cyc), row in zip(keys, host):
                n = float(row[2])
                l1, l2 = (float(row[0]) / n, float(row[1]) / n) if n else (float("nan"), float("nan"))
                out[kind][cyc] = {"l1": l1, "l2": l2, "l1_grey": l1 * 127.5, "n": int(n)}
        return out


def predictor_eval(predictor, batches: Iterable[Dict[str, Tensor]], specs: Sequence[MetricSpec], columns=None,
                   capacity: int = 65536) -> Dict[str, object]:
    """``train_pgm.eval_epoch`` (train_pgm.py:175-249) on factual images through the same accumulator: the natural check after
    ``PredictorTrainStep``.  ``batches``: any iterable of {"x", variable: [B, k]} dicts, or a ``DeviceLoader(..., train=False)``
    (batches {"x", "pa"}) with ``columns`` = {variable: column of "pa", or (first column, width)}."""
    acc = None
    for batch in batches:
        if columns is not None and "pa" in batch:
            pa = batch["pa"]
            obs = {"x": batch["x"]}
            for k, c in columns.items():
                lo, w = (c, 1) if isinstance(c, int) else c
                obs[k] = pa[:, lo:lo + w]
        else:
            obs = dict(batch)
        if acc is None:
            x = obs["x"]
            acc = MetricAccumulator(specs, capacity, x.device if x.is_cuda else "cuda")
        acc.update_from(predictor, **obs)
    if acc is None:
        raise ValueError("predictor_eval: no batches")
    return acc.compute()
