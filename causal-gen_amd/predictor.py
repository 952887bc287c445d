"""Anticausal predictors and the counterfactual auxiliary loss without pyro -- the ``predictor`` / ``elbo_fn`` of train_cf.py.

``CNN`` is the reference's ``src/pgm/layers.py`` CNN with its parameter and buffer names, so that the ``encoder_*`` entries of a
reference PGM checkpoint load with ``strict=True``.  The predictors are frozen and in eval mode during counterfactual
fine-tuning (train_cf.py:123-124, dscm.py:23-24): every BatchNorm is a per-channel affine, folded once into the preceding conv /
linear (refreshed when a parameter or buffer changes), and each PGM's image heads run in ONE HIP launch per direction
(csrc/predictor.hip; one launch per LAYER on the tiled path that large images take, see ``_choose_path``): the trunk, the spatial
mean, the head MLP and the per-variable log-likelihood of flow_pgm.py's ``model_anticausal``.  Only the input gradient exists: ``d aux / d cf_x`` is what flows on into the HVAE.
(Training these predictors -- batch-statistic BatchNorm, parameter gradients, the optimiser step -- is ``predictor_train.PredictorTrainStep``;
nothing here has a training mode.)

``model_anticausal(**obs)`` returns the summed negative log-likelihood (what pyro's ``Trace_ELBO.differentiable_loss`` of the
anticausal model with the empty guide computes); ``AnticausalELBO`` hands it to ``DSCM.forward`` as ``elbo_fn``.
``encoder_a`` (UKBB age from two scalars) does not see the image: its eval forward stays host-side torch, as the parent SCMs' does
(pgm.py); ``PredictorTrainStep(scalar_heads=True)`` trains it on the device (csrc/predictor_mlp.inc).
"""
import ctypes
import os
from typing import Dict

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from . import _lib

_BN_EPS = 1e-5


class CNN(nn.Module):
    """layers.py:62-104 with the same module tree (``cnn.0`` ... ``cnn.18``, ``fc.0/1/3``).  Calling it runs the HIP kernel in
    eval mode (folded BatchNorm) and returns the raw head outputs; there is no training mode."""

    def __init__(self, in_shape=(1, 192, 192), width=16, num_outputs=1, context_dim=0):
        super().__init__()
        in_channels, res = in_shape[0], in_shape[1]
        self.in_shape, self.width, self.num_outputs, self.context_dim = tuple(in_shape), width, num_outputs, context_dim
        s = 2 if res > 64 else 1
        act = nn.LeakyReLU()
        layers = [nn.Conv2d(in_channels, width, 7, s, 3, bias=False), nn.BatchNorm2d(width), act,
                  nn.MaxPool2d(2, 2) if res > 32 else nn.Identity()]
        for ci, co, st in ((width, 2 * width, 2), (2 * width, 2 * width, 1), (2 * width, 4 * width, 2), (4 * width, 4 * width, 1),
                           (4 * width, 8 * width, 2)):
            layers += [nn.Conv2d(ci, co, 3, st, 1, bias=False), nn.BatchNorm2d(co), act]
        self.cnn = nn.Sequential(*layers)
        self.fc = nn.Sequential(nn.Linear(8 * width + context_dim, 8 * width, bias=False), nn.BatchNorm1d(8 * width), act,
                                nn.Linear(8 * width, num_outputs))
        self.eval()

    def train(self, mode: bool = True):
        return super().train(False)  # eval mode only: the predictors are frozen (train_cf.py:123-124)

    def _convs(self):
        return [(self.cnn[i], self.cnn[i + 1]) for i in (0, 4, 7, 10, 13, 16)]

    def _state_key(self, device):
        return (str(device),) + tuple(t._version for t in list(self.parameters()) + list(self.buffers())) + \
            tuple(t.data_ptr() for t in self.parameters())

    @torch.no_grad()
    def folded(self, device):
        """[(weight, bias)] x 8 on ``device``: the six convs and fc.0 with their BatchNorm folded in, then fc.3."""
        key = self._state_key(device)
        rt = self.__dict__.get("_rt")
        if rt is not None and rt[0] == key:
            return rt[1]

        def fold(w, bn):
            scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + _BN_EPS)
            wf = w.double() * scale.reshape(-1, *([1] * (w.dim() - 1)))
            bf = bn.bias.double() - bn.running_mean.double() * scale
            return wf.float().to(device).contiguous(), bf.float().to(device).contiguous()

        out = [fold(conv.weight, bn) for conv, bn in self._convs()]
        out.append(fold(self.fc[0].weight, self.fc[1]))
        out.append((self.fc[3].weight.detach().float().to(device).contiguous(), self.fc[3].bias.detach().float().to(device).contiguous()))
        self.__dict__["_rt"] = (key, out)
        return out

    def __deepcopy__(self, memo):
        import copy as _copy

        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k != "_rt":  # the folded device copy is runtime state: rebuilt on first use
                new.__dict__[k] = _copy.deepcopy(v, memo)
        return new

    def path(self, x: Tensor) -> str:
        """The placement a call with this image batch takes now: "fused", "workspace" or "tiled"."""
        kind = _lib.PRED_BERNOULLI if self.num_outputs == 1 else _lib.PRED_CATEGORICAL
        return _path_of([_Head(self, kind, False, None, None)], {"x": x}, 0.0)

    def forward(self, x: Tensor, y: Tensor = None) -> Tensor:
        kind = _lib.PRED_BERNOULLI if self.num_outputs == 1 else _lib.PRED_CATEGORICAL  # (outputs only: the kind sets no math)
        spec = _Head(self, kind, False, None, "y" if y is not None else None)
        obs = {"x": x}
        if y is not None:
            obs["y"] = y
        return _run_outputs([spec], obs, std_fixed=0.0)[0]


class MLP(nn.Module):
    """layers.py:46-59 (``encoder_a``): host-side torch in eval mode -- two scalars in, no image.  (Its training mode is
    ``cgen_mlp_train_*``, run by ``PredictorTrainStep(scalar_heads=True)`` on these very parameters.)"""

    def __init__(self, num_inputs=1, width=32, num_outputs=1):
        super().__init__()
        act = nn.LeakyReLU()
        self.mlp = nn.Sequential(nn.Linear(num_inputs, width, bias=False), nn.BatchNorm1d(width), act,
                                 nn.Linear(width, width, bias=False), nn.BatchNorm1d(width), act, nn.Linear(width, num_outputs))
        self.eval()

    def train(self, mode: bool = True):
        return super().train(False)

    def forward(self, x):
        return self.mlp(x)


class _ScalarHead:
    """One scalar head of a PGM: its MLP, the variable it scores as Normal(loc, f(logscale)) and the observed variables it reads,
    in the order they are concatenated."""

    def __init__(self, mlp, var, inputs, tanh_loc=False):
        self.mlp, self.var, self.inputs, self.tanh_loc = mlp, var, tuple(inputs), tanh_loc


class _Head:
    """One image head of a PGM: its CNN, the variable it scores, its likelihood and the context variable (or None)."""

    def __init__(self, cnn, kind, tanh_loc, var, ctx_var):
        self.cnn, self.kind, self.tanh_loc, self.var, self.ctx_var = cnn, kind, tanh_loc, var, ctx_var


def _col(v: Tensor, B: int, device) -> Tensor:
    return v.detach().reshape(B, -1).float().to(device).contiguous()


def _layered() -> bool:
    return os.environ.get("CGEN_PREDICTOR_LAYERED", "0") == "1"


def fill_head(r, hd, xshape, std_fixed, ctx_width=None):
    """Geometry and likelihood fields of the ``PredHead`` `r` for head `hd` on images of `xshape` ([B, C, R, R]), refusing another
    input shape than the head was built for.  `ctx_width`: the columns of the context buffer the caller points ``y`` at (None: it
    reads no context); the weight and ``y`` / ``obs`` pointers are the caller's."""
    cnn = hd.cnn
    if tuple(cnn.in_shape) != tuple(xshape[1:]):
        raise ValueError(f"predictor head for {hd.var}: built for input {cnn.in_shape}, got {tuple(xshape[1:])}")
    if ctx_width is not None and ctx_width != cnn.context_dim:
        raise ValueError(f"predictor head for {hd.var}: context {hd.ctx_var} has {ctx_width} columns, expected {cnn.context_dim}")
    r.c, r.res, r.width, r.nout, r.ctx = xshape[1], xshape[-1], cnn.width, cnn.num_outputs, cnn.context_dim
    r.kind, r.tanh_loc, r.std_fixed = hd.kind, int(hd.tanh_loc), float(std_fixed)


def _records(heads, obs, std_fixed, need_obs, need_ctx=True):
    """ctypes head records + the tensors they point into (kept alive by the caller)."""
    x = obs["x"]
    B, dev = x.shape[0], x.device
    recs = (_lib.PredHead * len(heads))()
    keep = []
    for r, hd in zip(recs, heads):
        y = _col(obs[hd.ctx_var], B, dev) if hd.cnn.context_dim and need_ctx else None
        fill_head(r, hd, x.shape, std_fixed, None if y is None else y.shape[1])
        wb = hd.cnn.folded(dev)
        keep.append(wb)  # the records hold raw pointers into these: a refold between forward and backward must not free them
        for i, (w, b) in enumerate(wb):
            r.w[i], r.b[i] = w.data_ptr(), b.data_ptr()
        if y is not None:
            keep.append(y)
            r.y = y.data_ptr()
        if need_obs:
            o = _col(obs[hd.var], B, dev)
            keep.append(o)
            r.obs, r.obs_stride = o.data_ptr(), o.shape[1]
    return recs, keep


def _choose_path(lib, recs) -> str:
    """Where a call runs: "fused" (activation stack in LDS, one workgroup per image), "workspace" (the same kernel with the stack
    in global memory) or "tiled" (one launch per layer over tile x image x head).  CGEN_PREDICTOR_LAYERED=1 forces the workspace
    path; else CGEN_PREDICTOR_TILED=1 takes the tiled path wherever it is supported and CGEN_PREDICTOR_TILED=0 never does; unset,
    the fused path is taken where it fits, else the tiled one where supported, else the workspace."""
    nh = len(recs)
    if _layered():
        return "workspace"
    tiled = os.environ.get("CGEN_PREDICTOR_TILED")
    tiled_ok = tiled != "0" and lib._raw_cgen_predictor_tiled_supported(recs, nh) == 1
    if tiled == "1" and tiled_ok:
        return "tiled"
    if lib._raw_cgen_predictor_supported(recs, nh) == 1:
        return "fused"
    return "tiled" if tiled_ok else "workspace"


def _cached(owner, key, need, dev):
    ws = owner.__dict__.get(key) if owner is not None else None
    if ws is None or ws.numel() < need or ws.device != dev:
        ws = torch.empty(need, dtype=torch.float32, device=dev)
        if owner is not None:
            owner.__dict__[key] = ws
    return ws


def _route(heads_owner, recs, n, dev):
    """(path, workspace or None) of a call; the workspaces are cached on the owner (one per placement).  A backward uses the
    pair its forward got, whatever the environment says by then."""
    lib = _lib.require_gpu()
    path = _choose_path(lib, recs)
    if path == "fused":
        return path, None
    need = _lib.i64(0)
    if path == "tiled":
        lib.predictor_tiled_workspace(recs, len(recs), n, ctypes.byref(need))
        return path, _cached(heads_owner, "_ws_tiled", need.value, dev)
    lib.predictor_workspace(recs, len(recs), ctypes.byref(need))
    return path, _cached(heads_owner, "_ws", need.value * n, dev)


def _fwd(lib, route, recs, n, x, terms, outs, loss):
    path, ws = route
    t, o, l = (v.data_ptr() if v is not None else None for v in (terms, outs, loss))
    stream = torch.cuda.current_stream(x.device).cuda_stream
    if path == "tiled":
        lib.predictor_tiled_fwd(recs, len(recs), n, x.data_ptr(), ws.data_ptr(), ws.numel(), t, o, l, stream)
    else:
        lib.predictor_fwd(recs, len(recs), n, x.data_ptr(), ws.data_ptr() if ws is not None else None, t, o, l, stream)


def _bwd(lib, route, recs, n, x, coef, dx):
    path, ws = route
    stream = torch.cuda.current_stream(x.device).cuda_stream
    if path == "tiled":
        lib.predictor_tiled_bwd(recs, len(recs), n, x.data_ptr(), ws.data_ptr(), ws.numel(), coef.data_ptr(), dx.data_ptr(), stream)
    else:
        lib.predictor_bwd(recs, len(recs), n, x.data_ptr(), ws.data_ptr() if ws is not None else None, coef.data_ptr(), dx.data_ptr(),
                          stream)


def _path_of(heads, obs, std_fixed) -> str:
    lib = _lib.require_gpu()
    x = _prep_x(obs["x"])
    recs, keep = _records(heads, dict(obs, x=x), std_fixed, need_obs=False, need_ctx=False)
    return _choose_path(lib, recs)


def _prep_x(x: Tensor) -> Tensor:
    if not x.is_cuda:
        x = x.cuda()
    return x.detach().float().contiguous()


def _run_outputs(heads, obs, std_fixed, owner=None):
    """Raw head outputs, one [B, nout] tensor per head (no likelihood)."""
    lib = _lib.require_gpu()
    x = _prep_x(obs["x"])
    obs = dict(obs, x=x)
    B = x.shape[0]
    recs, keep = _records(heads, obs, std_fixed, need_obs=False)
    route = _route(owner, recs, B, x.device)
    outs = torch.empty(len(heads), B, _lib.PRED_MAX_OUT, device=x.device)
    _fwd(lib, route, recs, B, x, None, outs, None)
    return [outs[h, :, :hd.cnn.num_outputs] for h, hd in enumerate(heads)]


class _PredictorNLL(torch.autograd.Function):
    """sum over samples and image heads of -log p(obs | x): forward and input gradient are one launch each."""

    @staticmethod
    def forward(ctx, x, owner, heads, obs, std_fixed):
        lib = _lib.require_gpu()
        xd = _prep_x(x)
        B = xd.shape[0]
        full = dict(obs, x=xd)
        recs, keep = _records(heads, full, std_fixed, need_obs=True)
        route = _route(owner, recs, B, xd.device)
        terms = torch.empty(B, len(heads), device=xd.device)
        loss = torch.empty(1, device=xd.device)
        _fwd(lib, route, recs, B, xd, terms, None, loss)
        ctx.state = (recs, keep, xd, route, x.device, x.dtype)
        return loss[0].to(x.device)

    @staticmethod
    def backward(ctx, g):
        lib = _lib.require_gpu()
        recs, keep, xd, route, xdev, xdt = ctx.state
        coef = g.detach().reshape(1).float().to(xd.device).contiguous()
        dx = torch.empty_like(xd)
        _bwd(lib, route, recs, xd.shape[0], xd, coef, dx)
        return dx.to(device=xdev, dtype=xdt), None, None, None, None


class _AnticausalPredictor(nn.Module):
    """Common surface of the three predictors: model_anticausal / guide_pass / predict / load_reference_state_dict."""

    def __init__(self, args):
        super().__init__()
        self.std_fixed = float(getattr(args, "std_fixed", 0.0) or 0.0)

    def f(self, x: Tensor) -> Tensor:
        return self.std_fixed * torch.ones_like(x) if self.std_fixed > 0 else F.softplus(x)

    def _heads(self):
        raise NotImplementedError

    def _scalar_heads(self):
        """The heads that see no image (``predictor_train.PredictorTrainStep(scalar_heads=True)`` trains them): none by default."""
        return []

    def train(self, mode: bool = True):
        return super().train(False)

    def _host_nll(self, obs) -> Tensor:
        return None

    def model_anticausal(self, **obs) -> Tensor:
        """-sum_{samples, variables} log q(parent | x, ...) -- differentiable w.r.t. obs["x"]."""
        heads = self._heads()
        aux = {k: v for k, v in obs.items() if k != "x" and isinstance(v, Tensor)}
        nll = _PredictorNLL.apply(obs["x"], self, heads, aux, self.std_fixed)
        host = self._host_nll(obs)
        return nll if host is None else nll + host.to(nll.device)

    @torch.no_grad()
    def nll_terms(self, **obs) -> Dict[str, Tensor]:
        """Per-sample -log q of each image head ({variable: [B]}), as the forward launch writes them (no autograd)."""
        lib = _lib.require_gpu()
        heads = self._heads()
        x = _prep_x(obs["x"])
        B = x.shape[0]
        recs, keep = _records(heads, dict(obs, x=x), self.std_fixed, need_obs=True)
        route = _route(self, recs, B, x.device)
        terms = torch.empty(B, len(heads), device=x.device)
        _fwd(lib, route, recs, B, x, terms, None, None)
        return {hd.var: terms[:, h] for h, hd in enumerate(heads)}

    def path(self, x: Tensor) -> str:
        """The placement a call with this image batch takes now: "fused", "workspace" or "tiled"."""
        return _path_of(self._heads(), {"x": x}, self.std_fixed)

    def guide_pass(self, **obs) -> None:
        pass

    def _outputs(self, obs) -> Dict[str, Tensor]:
        heads = self._heads()
        outs = _run_outputs(heads, obs, self.std_fixed, owner=self)
        return {hd.var: o for hd, o in zip(heads, outs)}

    def _host_outputs(self, obs) -> Dict[str, Tensor]:
        return {}

    @torch.no_grad()
    def raw_outputs(self, **obs) -> Dict[str, Tensor]:
        """What ``predict`` starts from, before its sigmoid / softmax / tanh: {variable: [B, nout] raw head outputs}, each a view
        (row stride CGEN_PRED_MAX_OUT) into the forward launch's output buffer, plus the locs of the host-side heads
        (``FlowPredictor``: "age").  ``cf_eval.MetricAccumulator.update_from`` hands these rows to the metric kernel in place."""
        out = self._outputs(obs)
        out.update(self._host_outputs(obs))
        return out

    def load_reference_state_dict(self, sd: Dict[str, Tensor]):
        """Load the anticausal predictors of a reference PGM checkpoint (train_cf.py:302-308 loads a whole FlowPGM as the predictor):
        exactly its ``encoder_*`` keys, strictly; the parent mechanisms' keys are dropped and returned (pgm.py loads those)."""
        kept = {k: v for k, v in sd.items() if k.split(".")[0].startswith("encoder_")}
        dropped = sorted(set(sd) - set(kept))
        self.load_state_dict(kept, strict=True)
        return dropped

    def __deepcopy__(self, memo):
        import copy as _copy

        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k not in ("_ws", "_ws_tiled"):  # runtime workspaces
                new.__dict__[k] = _copy.deepcopy(v, memo)
        return new


class MorphoMNISTPredictor(_AnticausalPredictor):
    """flow_pgm.py:355-441: q(t | x, i), q(i | x) Normal(tanh(loc), f(logscale)); q(y | x) OneHotCategorical(softmax)."""

    def __init__(self, args):
        super().__init__(args)
        shape = (args.input_channels, args.input_res, args.input_res)
        self.encoder_t = CNN(shape, num_outputs=2, context_dim=1, width=8)
        self.encoder_i = CNN(shape, num_outputs=2, width=8)
        self.encoder_y = CNN(shape, num_outputs=10, width=8)

    def _heads(self):
        return [_Head(self.encoder_t, _lib.PRED_NORMAL, True, "thickness", "intensity"),
                _Head(self.encoder_i, _lib.PRED_NORMAL, True, "intensity", None),
                _Head(self.encoder_y, _lib.PRED_CATEGORICAL, False, "digit", None)]

    def predict(self, **obs) -> Dict[str, Tensor]:
        o = self._outputs(obs)
        return {"thickness": torch.tanh(o["thickness"][:, :1]), "intensity": torch.tanh(o["intensity"][:, :1]),
                "digit": F.softmax(o["digit"], dim=-1)}


class ColourMNISTPredictor(_AnticausalPredictor):
    """flow_pgm.py:460-523: q(y | x), q(c | x) OneHotCategorical(softmax)."""

    def __init__(self, args):
        super().__init__(args)
        shape = (args.input_channels, args.input_res, args.input_res)
        self.encoder_y = CNN(shape, num_outputs=10, width=8)
        self.encoder_c = CNN(shape, num_outputs=10, width=8)

    def _heads(self):
        return [_Head(self.encoder_y, _lib.PRED_CATEGORICAL, False, "digit", None),
                _Head(self.encoder_c, _lib.PRED_CATEGORICAL, False, "colour", None)]

    def predict(self, **obs) -> Dict[str, Tensor]:
        o = self._outputs(obs)
        return {"digit": F.softmax(o["digit"], dim=-1), "colour": F.softmax(o["colour"], dim=-1)}


class FlowPredictor(_AnticausalPredictor):
    """flow_pgm.py:150-303 (UKBB): q(v | x), q(b | x, v) Normal(loc, f(logscale)) -- no tanh; q(s | x, b), q(m | x)
    Bernoulli(sigmoid); q(a | b, v) Normal from the host-side MLP."""

    def __init__(self, args):
        super().__init__(args)
        shape = (args.input_channels, args.input_res, args.input_res)
        self.encoder_s = CNN(shape, num_outputs=1, context_dim=1)
        self.encoder_m = CNN(shape, num_outputs=1)
        self.encoder_a = MLP(num_inputs=2, num_outputs=2)
        self.encoder_b = CNN(shape, num_outputs=2, context_dim=1)
        self.encoder_v = CNN(shape, num_outputs=2)

    def _heads(self):
        return [_Head(self.encoder_v, _lib.PRED_NORMAL, False, "ventricle_volume", None),
                _Head(self.encoder_b, _lib.PRED_NORMAL, False, "brain_volume", "ventricle_volume"),
                _Head(self.encoder_s, _lib.PRED_BERNOULLI, False, "sex", "brain_volume"),
                _Head(self.encoder_m, _lib.PRED_BERNOULLI, False, "mri_seq", None)]

    def _scalar_heads(self):
        return [_ScalarHead(self.encoder_a, "age", ("brain_volume", "ventricle_volume"))]  # (the order _age concatenates them in)

    def _age(self, obs):
        dev = self.encoder_a.mlp[0].weight.device
        B = obs["x"].shape[0]
        ctx = torch.cat([obs["brain_volume"].reshape(B, 1), obs["ventricle_volume"].reshape(B, 1)], dim=-1).float().to(dev)
        return self.encoder_a(ctx).chunk(2, dim=-1)

    def _host_nll(self, obs) -> Tensor:
        a_loc, a_logscale = self._age(obs)
        age = obs["age"].reshape(a_loc.shape).float().to(a_loc.device)
        return -torch.distributions.Normal(a_loc, self.f(a_logscale)).log_prob(age).sum()

    def _host_outputs(self, obs) -> Dict[str, Tensor]:
        return {"age": self._age(obs)[0]}

    def predict(self, **obs) -> Dict[str, Tensor]:
        o = self._outputs(obs)
        a_loc, _ = self._age(obs)
        return {"sex": torch.sigmoid(o["sex"]), "mri_seq": torch.sigmoid(o["mri_seq"]), "age": a_loc,
                "brain_volume": o["brain_volume"][:, :1], "ventricle_volume": o["ventricle_volume"][:, :1]}


def make_predictor(args) -> _AnticausalPredictor:
    """The predictor train_cf.py builds for ``args.dataset``."""
    ds = getattr(args, "dataset", "")
    if "ukbb" in ds:
        return FlowPredictor(args)
    if "morphomnist" in ds:
        return MorphoMNISTPredictor(args)
    if "cmnist" in ds:
        return ColourMNISTPredictor(args)
    if "mimic" in ds:
        # (mimic's predictor exists -- predictor_resnet.ChestPredictor(args), constructed directly; this factory keeps its answer)
        raise NotImplementedError("ChestPGM's anticausal predictors (ResNet-18 heads) are not implemented on this backend")
    raise ValueError(f"no anticausal predictor for dataset {ds!r}")


class AnticausalELBO:
    """Drop-in for train_cf.py's ``elbo_fn`` (``TraceStorage_ELBO`` over ``model_anticausal`` with the empty ``guide_pass``):
    ``differentiable_loss(model, guide, **cfs)`` = -sum of the anticausal log-likelihoods, differentiable w.r.t. cfs["x"]."""

    def differentiable_loss(self, model, guide, **cfs) -> Tensor:
        if guide is not None:
            guide(**cfs)
        return model(**cfs)
