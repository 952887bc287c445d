"""Training the anticausal predictors on the GPU -- stage two of the reference pipeline (``src/pgm/train_pgm.py:111-170``,
``sup_epoch`` with ``--setup sup_aux``) as a fixed launch sequence:

    training forward (batch-statistic BatchNorm, csrc/predictor_train.inc) -> parameter gradients of loss / B ->
    global grad-norm -> clip at ``grad_clip`` / NaN-loss skip (on device) -> fused AdamW + EMA -> step counter commit

``loss`` is ``model_anticausal``'s summed negative log-likelihood of the trained heads divided by the batch size; the optimiser is
the reference's ``AdamW(lr, betas, eps, wd)`` under ``LambdaLR(linear_warmup(lr_warmup_steps))`` with ``clip_grad_norm_`` and
``EMA(beta=ema_rate)``.  The step tail is ``TrainStep``'s (csrc/optim.hip) and the skeleton around it -- constructor, ``_optim``,
``_run``, the staging of ``step``, the data-set half of ``step_from``, the checkpoint pair -- is ``step_tail.ImageSupStep``'s, shared
with ``ChestPredictorTrainStep``; this module has the flattening, the head records and the launches.  The float buffers (the BatchNorm running statistics)
are averaged into the EMA copy with the same device-derived decay, as ``utils.EMA`` does, integer buffers are not.  There is no
host synchronisation inside a step and the whole step is captured into one hipGraph after an eager first step.

Only this class trains: ``CNN.train()``, ``MLP.train()`` and the predictors' ``train()`` still force eval mode, ``model_anticausal``
and every eval route are unchanged.  By default the image heads alone are trained.  ``scalar_heads=True`` adds the heads that see no
image (``_AnticausalPredictor._scalar_heads()``: ``FlowPredictor.encoder_a``, UKBB age from two scalars; csrc/predictor_mlp.inc,
one launch each way): their parameters and statistics follow the image heads' in the flat vectors, their terms join the loss, and
the gradient norm, the clip, AdamW and both EMAs run over everything together, as ``clip_grad_norm_(model.parameters())`` does.

``step_from(ds, index)`` builds the batch on the device inside the captured step from a ``data.DeviceDataset`` whose ``pa`` holds
EVERY variable of the PGM (not only the HVAE's context), with the columns named at construction (``columns=``).
"""
import ctypes as C

import torch

from . import _lib
from .predictor import CNN, _Head, _prep_x, fill_head
from .step_tail import Flat, ImageSupStep, flatten

BN_MOMENTUM = 0.1  # nn.BatchNorm's default, what layers.py builds


class _Flat(Flat):
    """The trained heads of one predictor with their parameters and float buffers flattened (online model or EMA copy): the image
    heads, then -- with `scalar_heads` -- the scalar ones, so that the image heads' offsets are the same either way."""

    def __init__(self, pred, dev, scalar_heads=False):
        pred.to(dev)
        self.pred = pred
        if isinstance(pred, CNN):
            kind = _lib.PRED_BERNOULLI if pred.num_outputs == 1 else _lib.PRED_CATEGORICAL
            self.heads, prefixes = [_Head(pred, kind, False, "obs", "y" if pred.context_dim else None)], [""]
            self.std_fixed = 0.0
            self.scalars = []
        else:
            self.heads = pred._heads()
            names = {id(m): n for n, m in pred.named_modules()}
            prefixes = [names[id(hd.cnn)] + "." for hd in self.heads]
            self.std_fixed = float(pred.std_fixed)
            self.scalars = pred._scalar_heads() if scalar_heads else []
            prefixes += [names[id(sh.mlp)] + "." for sh in self.scalars]
        mods = self.cnns() + [sh.mlp for sh in self.scalars]
        super().__init__([(pre + n, p) for pre, m in zip(prefixes, mods) for n, p in m.named_parameters()], dev)
        named = [(pre + n, b) for pre, m in zip(prefixes, mods) for n, b in m.named_buffers() if b.is_floating_point()]
        self.bnames, self.bufs = [n for n, _ in named], [b for _, b in named]
        self.flat_b, self.b_off = flatten(self.bufs, dev)

    def cnns(self):
        return [hd.cnn for hd in self.heads]

    def variables(self):
        """every observed / context variable the trained heads read, in first-use order"""
        out = []
        for hd in self.heads:
            out += [hd.var, hd.ctx_var]
        for sh in self.scalars:
            out += [sh.var, *sh.inputs]
        return list(dict.fromkeys(v for v in out if v is not None))

    def invalidate(self):
        """The kernels write parameters and statistics through raw pointers, which the version counters ``CNN.folded`` keys its
        cache on do not see: drop the folded copies so that the next eval call folds the new values."""
        for cnn in self.cnns():
            cnn.__dict__.pop("_rt", None)


class PredictorTrainStep(ImageSupStep):
    """``state_dict()``'s optimiser state is in ``named_parameters`` order of the trained heads: image heads, then scalar heads."""
    NORM_BLOCKS = 1024

    def __init__(self, pred, lr=1e-4, wd=0.1, betas=(0.9, 0.999), eps=1e-8, grad_clip=200.0, lr_warmup_steps=1, ema_rate=0.999,
                 ema=True, use_graph=True, ema_update_after=100, device="cuda", scalar_heads=False, columns=None):
        self.scalar_heads = scalar_heads
        super().__init__(pred, columns, lr=lr, wd=wd, betas=betas, eps=eps, grad_clip=grad_clip, lr_warmup_steps=lr_warmup_steps,
                         ema_rate=ema_rate, ema=ema, use_graph=use_graph, ema_update_after=ema_update_after, device=device)
        widths = {c.width for c in self._on.cnns()}
        if len(widths) != 1:
            raise ValueError(f"PredictorTrainStep needs image heads of one width, got {sorted(widths)}")
        self._rng = None  # own Philox state {seed, offset} of step_from's crop / flip draws

    # -- pieces -------------------------------------------------------------------------------------------
    def _flatten(self, pred, dev):
        return _Flat(pred, dev, self.scalar_heads)

    def _variables(self):
        return self._on.variables()

    def _check_batch(self, B):
        if B < 2:
            raise ValueError("PredictorTrainStep: train-mode BatchNorm needs a batch of at least 2 images")

    def _build(self, x, at, dense):
        """Head records, workspaces and coefficient of a batch shape reading the static image `x`.  ``at(var)`` = (address, row
        stride in floats, width) of a variable's rows; ``dense[var]``: the contiguous [B, k] buffer of a context variable (None:
        the rows are strided, and ``_load`` copies each context out densely inside the step)."""
        dev, on, B = self.device, self._on, int(x.shape[0])
        if dense is None:
            dense = {hd.ctx_var: torch.empty((B, at(hd.ctx_var)[2]), device=dev) for hd in on.heads if hd.ctx_var is not None}
        recs = (_lib.PredTrainHead * len(on.heads))()
        g_of = {id(p): self.flat_g.data_ptr() + 4 * o for p, o in zip(on.params, on.p_off)}
        for r, hd in zip(recs, on.heads):
            cnn, h = hd.cnn, r.hd
            fill_head(h, hd, x.shape, on.std_fixed, dense[hd.ctx_var].shape[1] if cnn.context_dim else None)
            lin = [conv for conv, _ in cnn._convs()] + [cnn.fc[0], cnn.fc[3]]
            bns = [bn for _, bn in cnn._convs()] + [cnn.fc[1]]
            for i, m in enumerate(lin):
                h.w[i], r.gw[i] = m.weight.data_ptr(), g_of[id(m.weight)]
            h.b[7], r.gb = cnn.fc[3].bias.data_ptr(), g_of[id(cnn.fc[3].bias)]
            for i, bn in enumerate(bns):
                r.gamma[i], r.beta[i] = bn.weight.data_ptr(), bn.bias.data_ptr()
                r.ggamma[i], r.gbeta[i] = g_of[id(bn.weight)], g_of[id(bn.bias)]
                r.running_mean[i], r.running_var[i] = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
                r.num_batches_tracked[i] = bn.num_batches_tracked.data_ptr()
            if cnn.context_dim:
                h.y = dense[hd.ctx_var].data_ptr()
            h.obs, h.obs_stride, _ = at(hd.var)
        need = _lib.i64(0)
        self.lib.predictor_train_workspace(recs, len(recs), B, C.byref(need))
        ent = dict(recs=recs, B=B, x=x, dense=dense, ws=torch.empty(need.value, device=dev), terms=torch.empty(B, len(recs), device=dev),
                   coef=torch.full((1,), 1.0 / B, device=dev), scalars=[])
        for sh in on.scalars:
            m = sh.mlp.mlp
            r = _lib.MlpTrainHead()
            r.nin, r.width, r.tanh_loc, r.std_fixed = m[0].in_features, m[0].out_features, int(sh.tanh_loc), on.std_fixed
            k = 0
            for var in sh.inputs:
                ptr, stride, width = at(var)
                for c in range(width):
                    if k < _lib.MLP_MAX_IN:
                        r.in_[k], r.in_stride[k] = ptr + 4 * c, stride
                    k += 1
            if k != r.nin:
                raise ValueError(f"predictor head for {sh.var}: inputs {sh.inputs} have {k} columns, expected {r.nin}")
            r.obs, r.obs_stride, _ = at(sh.var)
            for i, j in enumerate((0, 3, 6)):
                r.w[i], r.gw[i] = m[j].weight.data_ptr(), g_of[id(m[j].weight)]
            r.bias, r.gb = m[6].bias.data_ptr(), g_of[id(m[6].bias)]
            for i, j in enumerate((1, 4)):
                r.gamma[i], r.beta[i], r.ggamma[i], r.gbeta[i] = m[j].weight.data_ptr(), m[j].bias.data_ptr(), g_of[id(m[j].weight)], g_of[id(m[j].bias)]
                r.running_mean[i], r.running_var[i] = m[j].running_mean.data_ptr(), m[j].running_var.data_ptr()
                r.num_batches_tracked[i] = m[j].num_batches_tracked.data_ptr()
            self.lib.mlp_train_workspace(C.byref(r), B, C.byref(need))
            ent["scalars"].append((r, torch.empty(need.value, device=dev), torch.empty(B, device=dev)))
        return ent

    def _static_for(self, obs):
        x = _prep_x(obs["x"])
        self._check_batch(int(x.shape[0]))
        return self._stage(x, obs)

    def _load(self, ent):
        """step_from's batch, inside the step: the next crop / flip draws, one augment launch into the static image with the
        parents rows gathered on the side, and the dense copies of the context columns"""
        st = self._stream()
        if ent["train"]:
            self.lib.rng_advance(self._rng.data_ptr(), 1, st)
        # (one channel: NHWC and planar are the same memory and the NHWC launch serves)
        (self.lib.batch_augment if ent["x"].shape[1] == 1 else self.lib.batch_augment_planar)(C.byref(ent["aug"]), st)
        for var, dst in ent["dense"].items():
            c0, k = self.columns[var]
            dst.copy_(ent["pa"][:, c0:c0 + k])

    def _fwd_bwd(self, ent, dx=None):
        st = self._stream()
        recs, B, ws = ent["recs"], ent["B"], ent["ws"]
        self.lib.predictor_train_fwd(recs, len(recs), B, ent["x"].data_ptr(), ws.data_ptr(), ws.numel(), BN_MOMENTUM, ent["terms"].data_ptr(),
                                     None, self.out3.data_ptr() + 4, st)
        for r, sws, terms in ent["scalars"]:  # (adds its terms to the image heads' sum: no launch for the addition)
            self.lib.mlp_train_fwd(C.byref(r), B, sws.data_ptr(), sws.numel(), BN_MOMENTUM, terms.data_ptr(), self.out3.data_ptr() + 4, st)
        self.lib.predictor_train_bwd(recs, len(recs), B, ent["x"].data_ptr(), ws.data_ptr(), ws.numel(), ent["coef"].data_ptr(),
                                     None if dx is None else dx.data_ptr(), st)
        for r, sws, _ in ent["scalars"]:
            self.lib.mlp_train_bwd(C.byref(r), B, sws.data_ptr(), sws.numel(), ent["coef"].data_ptr(), st)
        torch.mul(self.out3[1:2], 1.0 / B, out=self.res[0:1])

    def _ema_only(self):
        # EMA of the running statistics: lr = wd = 0 and a zero gradient leave the buffers as they are
        on = self._on
        return [(on.flat_b.data_ptr(), self._ema.flat_b.data_ptr(), on.flat_b.numel())] if self._ema is not None and on.flat_b.numel() else ()

    def _fwd_bwd_optim(self, ent):
        if "aug" in ent:
            self._load(ent)
        super()._fwd_bwd_optim(ent)

    # -- public -------------------------------------------------------------------------------------------
    def step(self, **obs):
        """One optimiser step on a batch (``x`` and every variable the trained heads score or condition on; with ``scalar_heads``
        that includes ``age``).  Returns the device scalars ``{"loss": mean loss, "grad_norm": norm before clipping}``; nothing
        is read back."""
        return self._run(*self._static_for(obs))

    def step_from(self, ds, index, train=True, draws_out=None):
        """One optimiser step on rows ``index`` (device int64 vector) of a ``data.DeviceDataset`` whose ``pa`` holds every variable
        of the PGM in the columns named at construction.  Inside the captured step: the class's own Philox state (seeded from
        ``torch.initial_seed()``) moves on by one, ONE augment launch writes the static image (contiguous f32 NCHW) and gathers the
        parents rows, and the heads read those rows in place.  The graph is keyed by the data set, its geometry and the batch size;
        ``draws_out`` (device int32 [B, 3]) receives the (oy, ox, flip) used, as in ``TrainStep.step_from``."""
        return self._run(*self._static_from(ds, index, train, draws_out))

    def loss_and_grads(self, dx=False, **obs):
        """(mean loss, {parameter name: d loss / d parameter}) of a batch; with ``dx`` also ``"x"``: d loss / d image.  Updates the
        running statistics (it IS a training forward) and nothing else."""
        _, ent = self._static_for(obs)
        gx = torch.empty_like(ent["x"]) if dx else None
        self._fwd_bwd(ent, gx)
        self._on.invalidate()
        grads = self._grads()
        if dx:
            grads["x"] = gx
        return self.res[0].clone(), grads
