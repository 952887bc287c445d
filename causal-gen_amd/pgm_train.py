"""Training the parent SCM on the GPU -- stage one of the reference pipeline (``src/pgm/train_pgm.py`` ``sup_epoch`` with
``--setup sup_pgm``: minimise ``-log p(parents)`` of ``svi_model`` under an empty guide) as a fixed launch sequence:

    log-likelihood terms and every parameter gradient of loss (csrc/pgm.hip, two launches) -> global grad-norm ->
    clip at ``grad_clip`` / NaN-loss skip (on device) -> fused AdamW + EMA -> step counter commit

``loss`` is ``pgm.nll``: minus the summed log-probability of every parent, divided by the batch size.  The optimiser is the
reference's ``AdamW(lr, betas, eps, wd)`` under ``LambdaLR(linear_warmup(lr_warmup_steps))`` with ``clip_grad_norm_`` and
``EMA(beta=ema_rate)``; the step tail (csrc/optim.hip) and everything around it that is not the PGM's own -- constructor, ``_run``,
checkpoint pair -- is ``step_tail.SupStep``'s, shared with ``PredictorTrainStep`` and ``ChestPredictorTrainStep``.  There is no host
synchronisation inside a step, nothing is read back, and the step is captured into one hipGraph per batch shape after an eager
first step.  The mechanisms come from ``pgm.mechanisms()``, the list ``pgm.log_prob`` is driven by, so the host density is the
oracle of this path.  The base ``*_base_loc`` / ``*_base_scale`` buffers are not trained.

A PGM the kernel does not serve (a hidden width above 64, more than three hidden layers, more than eight bins, another
activation) raises ``ValueError``; nothing falls back to host torch.
"""
import ctypes as C

import torch
from torch import nn

from . import _lib
from .pgm import ConditionalAffine, DenseNN, LinearSpline
from .step_tail import Flat, SupStep, check_index

_KINDS = {"bernoulli": _lib.PGM_BERNOULLI, "categorical": _lib.PGM_CATEGORICAL, "spline": _lib.PGM_SPLINE, "affine": _lib.PGM_AFFINE,
          "gumbel_max": _lib.PGM_GUMBEL_MAX}


def _act_of(f):
    if isinstance(f, nn.LeakyReLU) and abs(f.negative_slope - 0.1) < 1e-12:
        return _lib.PGM_LEAKY_RELU
    if isinstance(f, nn.GELU) and getattr(f, "approximate", "none") == "none":
        return _lib.PGM_GELU
    if isinstance(f, nn.Sigmoid):
        return _lib.PGM_SIGMOID
    raise ValueError(f"PgmTrainStep: the kernel serves LeakyReLU(0.1), exact GELU and Sigmoid, not {f!r}")


def default_columns(pgm):
    """{variable: first column} and the table width when the variables sit side by side in ``pgm.variables`` order, a one-hot
    variable taking as many columns as it has classes."""
    width = {m.var: (m.module.shape[-1] if m.kind == "categorical" else 1) for m in pgm.mechanisms()}
    cols, o = {}, 0
    for var in pgm.variables:
        cols[var] = o
        o += width[var]
    return cols, o


def _mlp_of(m):
    net = m.module.context_nn if isinstance(m.module, ConditionalAffine) else m.module
    if not isinstance(net, DenseNN):
        raise ValueError(f"PgmTrainStep: mechanism {m.var!r}: the kernel serves a DenseNN context network, not {type(net).__name__}")
    return net


def build_records(pgm, columns, ncol, grad_ptr=None):
    """The ``cgen_pgm_mech`` array of ``pgm.mechanisms()``.  ``grad_ptr``: {id(parameter): device address of its gradient}."""
    mechs = pgm.mechanisms()
    if not 1 <= len(mechs) <= _lib.PGM_MAX_MECH:
        raise ValueError(f"PgmTrainStep: the kernel serves 1..{_lib.PGM_MAX_MECH} mechanisms, this PGM has {len(mechs)}")
    recs = (_lib.PgmMech * len(mechs))()
    for r, m in zip(recs, mechs):
        if m.var not in columns:
            raise ValueError(f"PgmTrainStep: no column was named for variable {m.var!r}")
        r.kind, r.normalize, r.col = _KINDS[m.kind], int(m.normalize), int(columns[m.var])
        span, params = 1, []
        if m.kind in ("bernoulli", "categorical"):
            params = [m.module]
            if m.kind == "categorical":
                r.ncls = span = int(m.module.shape[-1])
                if not 2 <= r.ncls <= _lib.PGM_MAX_CLS:
                    raise ValueError(f"PgmTrainStep: mechanism {m.var!r}: {r.ncls} classes, the kernel serves 2..{_lib.PGM_MAX_CLS}")
        elif m.kind == "spline":
            sp = m.module
            if not isinstance(sp, LinearSpline) or sp.input_dim != 1:
                raise ValueError(f"PgmTrainStep: mechanism {m.var!r}: the kernel serves a one-dimensional LinearSpline")
            if not 2 <= sp.count_bins <= _lib.PGM_MAX_BINS:
                raise ValueError(f"PgmTrainStep: mechanism {m.var!r}: {sp.count_bins} bins, the kernel serves 2..{_lib.PGM_MAX_BINS}")
            r.bins, r.bound = int(sp.count_bins), float(sp.bound)
            params = [sp.unnormalized_widths, sp.unnormalized_heights, sp.unnormalized_derivatives, sp.unnormalized_lambdas]
        else:
            net = _mlp_of(m)
            hidden = [lin.out_features for lin in net.layers[:-1]]
            if not 1 <= len(hidden) <= _lib.PGM_MAX_HIDDEN:
                raise ValueError(f"PgmTrainStep: mechanism {m.var!r}: {len(hidden)} hidden layers, the kernel serves 1..{_lib.PGM_MAX_HIDDEN}")
            if max(hidden) > _lib.PGM_MAX_WIDTH:
                raise ValueError(f"PgmTrainStep: mechanism {m.var!r}: hidden widths {hidden}, the kernel serves widths up to {_lib.PGM_MAX_WIDTH}")
            if not 1 <= len(m.ctx) <= 2 or net.layers[0].in_features != len(m.ctx):
                raise ValueError(f"PgmTrainStep: mechanism {m.var!r}: a context of {net.layers[0].in_features} values over {len(m.ctx)} "
                                 "variables, the kernel serves one or two scalar context variables")
            nout = net.layers[-1].out_features
            if m.kind == "gumbel_max":
                r.ncls = int(nout)
                if not 2 <= r.ncls <= _lib.PGM_MAX_CLS:
                    raise ValueError(f"PgmTrainStep: mechanism {m.var!r}: {r.ncls} classes, the kernel serves 2..{_lib.PGM_MAX_CLS}")
            elif nout != 2:
                raise ValueError(f"PgmTrainStep: mechanism {m.var!r}: the context network must give (loc, log_scale), it gives {nout} values")
            r.nctx, r.nhidden, r.act = len(m.ctx), len(hidden), _act_of(net.f)
            for i, c in enumerate(m.ctx):
                if c not in columns:
                    raise ValueError(f"PgmTrainStep: no column was named for variable {c!r}")
                r.ctx_col[i] = int(columns[c])
            for i, w in enumerate(hidden):
                r.width[i] = int(w)
            for lin in net.layers:
                params += [lin.weight, lin.bias]
        if not 0 <= r.col <= ncol - span:
            raise ValueError(f"PgmTrainStep: variable {m.var!r}: columns {r.col}..{r.col + span - 1} do not fit a table of {ncol} columns")
        for i, p in enumerate(params):
            r.p[i] = p.data_ptr()
            if grad_ptr is not None:
                r.g[i] = grad_ptr[id(p)]
    return recs


class PgmTrainStep(SupStep):
    NORM_BLOCKS = 64

    def __init__(self, pgm, lr=1e-4, wd=0.1, betas=(0.9, 0.999), eps=1e-8, grad_clip=200.0, lr_warmup_steps=1, ema_rate=0.999, ema=True,
                 use_graph=True, ema_update_after=100, columns=None, ncol=None, device="cuda"):
        if columns is None:
            columns, width = default_columns(pgm)
            ncol = width if ncol is None else ncol
        self.columns = dict(columns)  # {variable: FIRST column} (a one-hot variable's width is its mechanism's)
        if ncol is None:
            raise ValueError("PgmTrainStep: `ncol` (the table's width) is needed with named columns")
        self.ncol = int(ncol)
        super().__init__(pgm, lr, wd, betas, eps, grad_clip, lr_warmup_steps, ema_rate, ema, use_graph, ema_update_after, device)
        on = self._on
        self.recs = build_records(pgm, self.columns, self.ncol, {id(p): self.flat_g.data_ptr() + 4 * o for p, o in zip(on.params, on.p_off)})
        self.nmech = len(self.recs)

    # -- pieces -------------------------------------------------------------------------------------------
    def _flatten(self, pgm, dev):
        return Flat(pgm.to(dev).named_parameters(), dev)

    def _entry(self, key, B, table, index):
        ent = self._statics.get(key)
        if ent is None:
            need = _lib.i64(0)
            self.lib.pgm_workspace(self.recs, self.nmech, B, C.byref(need))
            dev = self.device
            ent = self._statics[key] = dict(B=B, table=table, index=index, ws=torch.empty(max(need.value // 4, 1), device=dev),
                                            terms=torch.empty(B, self.nmech, device=dev), coef=torch.full((1,), -1.0 / B, device=dev))
        return ent

    def _static_for(self, obs):
        """The static table of a batch given by variable; `obs` is copied into it."""
        cols = {}
        for var, c0 in self.columns.items():
            if var not in self.model.variables:
                continue
            if var not in obs:
                raise KeyError(f"PgmTrainStep: observation {var!r} is missing")
            v = obs[var].detach()
            cols[var] = (c0, v.reshape(v.shape[0], -1).float())
        B = int(next(iter(cols.values()))[1].shape[0])
        key = ("obs", B)
        ent = self._statics.get(key)
        if ent is None:
            ent = self._entry(key, B, torch.zeros(B, self.ncol, device=self.device), None)
        for var, (c0, v) in cols.items():
            if v.shape[0] != B or c0 + v.shape[1] > self.ncol:
                raise ValueError(f"PgmTrainStep: observation {var!r} of shape {tuple(v.shape)} does not fit rows {B}, columns {c0}..")
            ent["table"][:, c0:c0 + v.shape[1]].copy_(v, non_blocking=v.is_cuda)
        return key, ent

    def _static_from(self, table, index):
        if table.dtype != torch.float32 or table.dim() != 2 or table.shape[1] != self.ncol or not table.is_contiguous() or table.device.type != "cuda":
            raise ValueError(f"PgmTrainStep.step_from: the table must be a contiguous f32 [N, {self.ncol}] device tensor")
        check_index(index, "PgmTrainStep.step_from")
        B = int(index.numel())
        key = ("from", table.data_ptr(), int(table.shape[0]), B)
        ent = self._statics.get(key)
        if ent is None:
            ent = self._entry(key, B, table, torch.zeros(B, dtype=torch.int64, device=self.device))
        ent["index"].copy_(index, non_blocking=True)
        return key, ent

    def _launch_args(self, ent):
        t, idx = ent["table"], ent["index"]
        return (self.recs, self.nmech, t.data_ptr(), self.ncol, int(t.shape[0]), None if idx is None else idx.data_ptr(), ent["B"],
                ent["terms"].data_ptr(), self.out3.data_ptr() + 4)

    def _fwd_bwd(self, ent):
        self.lib.pgm_nll_fwd_bwd(*self._launch_args(ent), ent["coef"].data_ptr(), ent["ws"].data_ptr(), ent["ws"].numel() * 4, self._stream())
        torch.div(self.out3[1:2], -float(ent["B"]), out=self.res[0:1])

    def _fwd(self, ent):
        self.lib.pgm_nll_fwd(*self._launch_args(ent), self._stream())
        torch.div(self.out3[1:2], -float(ent["B"]), out=self.res[0:1])

    # -- public -------------------------------------------------------------------------------------------
    def step(self, **obs):
        """One optimiser step on a batch given by variable (``[B, 1]`` columns, one-hot ``[B, k]``).  Returns the device scalars
        ``{"loss": mean loss, "grad_norm": norm before clipping}``; nothing is read back."""
        return self._run(*self._static_for(obs))

    def step_from(self, table, index):
        """One optimiser step on rows ``index`` (device int64 vector) of a device-resident f32 ``[N, ncol]`` table of parents whose
        columns were named at construction; the rows are gathered inside the captured step."""
        return self._run(*self._static_from(table, index))

    def loss(self, **obs):
        """Mean loss of a batch, forward only (``sup_epoch(is_train=False)``): a device scalar."""
        _, ent = self._static_for(obs)
        self._fwd(ent)
        return self.res[0].clone()

    def terms(self, **obs):
        """``[B, mechanisms]`` log-probability terms of a batch, in ``pgm.mechanisms()`` order (forward only)."""
        _, ent = self._static_for(obs)
        self._fwd(ent)
        return ent["terms"].clone()

    def loss_and_grads(self, **obs):
        """(mean loss, {parameter name: d loss / d parameter}) of a batch; changes no parameter."""
        _, ent = self._static_for(obs)
        self._fwd_bwd(ent)
        return self.res[0].clone(), self._grads()

    # -- checkpoint: also a reference checkpoint, whose ``encoder_*`` keys are dropped (``load_reference_state_dict``) -------------
    def _load_model(self, model, sd):
        model.load_reference_state_dict(sd)

    def _optimizer_state(self, sd):
        opt = sd.get("optimizer_state_dict")  # (absent, or torch's own layout, in a reference checkpoint: the moments stay)
        return opt if opt is not None and "exp_avg" in opt else None
