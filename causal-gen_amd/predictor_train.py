"""Training the anticausal predictors on the GPU -- stage two of the reference pipeline (``src/pgm/train_pgm.py:111-170``,
``sup_epoch`` with ``--setup sup_aux``) as a fixed launch sequence:

    training forward (batch-statistic BatchNorm, csrc/predictor_train.inc) -> parameter gradients of loss / B ->
    global grad-norm -> clip at ``grad_clip`` / NaN-loss skip (on device) -> fused AdamW + EMA -> step counter commit

``loss`` is ``model_anticausal``'s summed negative log-likelihood of the image heads divided by the batch size; the optimiser is
the reference's ``AdamW(lr, betas, eps, wd)`` under ``LambdaLR(linear_warmup(lr_warmup_steps))`` with ``clip_grad_norm_`` and
``EMA(beta=ema_rate)``.  The step tail is ``TrainStep``'s (csrc/optim.hip); the float buffers (the BatchNorm running statistics)
are averaged into the EMA copy with the same device-derived decay, as ``utils.EMA`` does, integer buffers are not.  There is no
host synchronisation inside a step and the whole step is captured into one hipGraph after an eager first step.

Only this class trains: ``CNN.train()`` and the predictors' ``train()`` still force eval mode, ``model_anticausal`` and every
eval route are unchanged.  ``FlowPredictor.encoder_a`` (UKBB age from two scalars) is a host MLP that sees no image: it is NOT
trained here and its ``age`` term is not part of this step's loss.
"""
import copy
import ctypes as C

import torch

from . import _lib
from .predictor import CNN, _Head, _prep_x
from .step_tail import NORM, Flat, HyperParams, StepTail, capture, check_warmup, flatten

BN_MOMENTUM = 0.1  # nn.BatchNorm's default, what layers.py builds


class _Flat(Flat):
    """The image heads of one predictor with their parameters and float buffers flattened (online model or EMA copy)."""

    def __init__(self, pred, dev):
        pred.to(dev)
        self.pred = pred
        if isinstance(pred, CNN):
            kind = _lib.PRED_BERNOULLI if pred.num_outputs == 1 else _lib.PRED_CATEGORICAL
            self.heads, prefixes = [_Head(pred, kind, False, "obs", "y" if pred.context_dim else None)], [""]
            self.std_fixed = 0.0
        else:
            self.heads = pred._heads()
            names = {id(m): n for n, m in pred.named_modules()}
            prefixes = [names[id(hd.cnn)] + "." for hd in self.heads]
            self.std_fixed = float(pred.std_fixed)
        super().__init__([(pre + n, p) for pre, hd in zip(prefixes, self.heads) for n, p in hd.cnn.named_parameters()], dev)
        named = [(pre + n, b) for pre, hd in zip(prefixes, self.heads) for n, b in hd.cnn.named_buffers() if b.is_floating_point()]
        self.bnames, self.bufs = [n for n, _ in named], [b for _, b in named]
        self.flat_b, self.b_off = flatten(self.bufs, dev)

    def cnns(self):
        return [hd.cnn for hd in self.heads]

    def invalidate(self):
        """The kernels write parameters and statistics through raw pointers, which the version counters ``CNN.folded`` keys its
        cache on do not see: drop the folded copies so that the next eval call folds the new values."""
        for cnn in self.cnns():
            cnn.__dict__.pop("_rt", None)


class PredictorTrainStep:
    NORM_BLOCKS = 1024

    def __init__(self, pred, lr=1e-4, wd=0.1, betas=(0.9, 0.999), eps=1e-8, grad_clip=200.0, lr_warmup_steps=1, ema_rate=0.999,
                 ema=True, use_graph=True, ema_update_after=100, device="cuda"):
        check_warmup(lr_warmup_steps)
        self.lib = _lib.require_gpu()
        dev = self.device = torch.device(device)
        # (no norm threshold in sup_epoch: only a non-finite norm or a NaN loss drops the step)
        self.hp = HyperParams(float(lr), (float(betas[0]), float(betas[1])), float(eps), float(wd), float(grad_clip), float("inf"),
                              int(lr_warmup_steps), float(ema_rate), int(ema_update_after))
        self.use_graph = use_graph
        self.ema_model = None
        if ema:
            self.ema_model = copy.deepcopy(pred)
            self.ema_model.requires_grad_(False)
            self._ema = _Flat(self.ema_model, dev)
        self.model = pred
        self._on = _Flat(pred, dev)
        widths = {c.width for c in self._on.cnns()}
        if len(widths) != 1:
            raise ValueError(f"PredictorTrainStep needs image heads of one width, got {sorted(widths)}")
        n = self._on.flat_p.numel()
        self.flat_g = torch.zeros(n, device=dev)
        self.tail = StepTail(self.lib, n, dev, self.NORM_BLOCKS)
        self.stats = self.tail.stats  # host read of the device-side step state (one sync)
        self.m, self.v, self.state, self.partial = self.tail.m, self.tail.v, self.tail.state, self.tail.partial
        self.out3 = torch.zeros(3, device=dev)  # [-, summed loss, 0]: what cgen_clip_decide tests for NaN
        self.res = torch.zeros(2, device=dev)   # [mean loss, gradient norm] of the last step
        self._statics, self._graphs = {}, {}
        self.it = 0

    # -- pieces -------------------------------------------------------------------------------------------
    def _cols(self, obs, B):
        """{variable: [B, k] f32} of every observed / context variable the heads read"""
        out = {}
        for hd in self._on.heads:
            for var in (hd.var, hd.ctx_var):
                if var is not None and var not in out:
                    if var not in obs:
                        raise KeyError(f"PredictorTrainStep: observation {var!r} is missing")
                    out[var] = obs[var].detach().reshape(B, -1).float()
        return out

    def _static_for(self, obs):
        """Static input buffers, head records, workspace and coefficient of a batch shape; `obs` is copied into the buffers."""
        x = _prep_x(obs["x"])
        B = int(x.shape[0])
        if B < 2:
            raise ValueError("PredictorTrainStep: train-mode BatchNorm needs a batch of at least 2 images")
        cols = self._cols(obs, B)
        key = tuple(x.shape)
        ent = self._statics.get(key)
        if ent is None:
            dev, on = self.device, self._on
            sx = torch.empty_like(x, device=dev)
            sc = {k: torch.empty(v.shape, device=dev) for k, v in cols.items()}
            recs = (_lib.PredTrainHead * len(on.heads))()
            g_of = {id(p): self.flat_g.data_ptr() + 4 * o for p, o in zip(on.params, on.p_off)}
            for r, hd in zip(recs, on.heads):
                cnn = hd.cnn
                if tuple(cnn.in_shape) != tuple(x.shape[1:]):
                    raise ValueError(f"predictor head for {hd.var}: built for input {cnn.in_shape}, got {tuple(x.shape[1:])}")
                h = r.hd
                h.c, h.res, h.width, h.nout, h.ctx = x.shape[1], x.shape[-1], cnn.width, cnn.num_outputs, cnn.context_dim
                h.kind, h.tanh_loc, h.std_fixed = hd.kind, int(hd.tanh_loc), on.std_fixed
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
                    if sc[hd.ctx_var].shape[1] != cnn.context_dim:
                        raise ValueError(f"predictor head for {hd.var}: context {hd.ctx_var} has {sc[hd.ctx_var].shape[1]} columns, "
                                         f"expected {cnn.context_dim}")
                    h.y = sc[hd.ctx_var].data_ptr()
                h.obs, h.obs_stride = sc[hd.var].data_ptr(), sc[hd.var].shape[1]
            need = _lib.i64(0)
            self.lib.predictor_train_workspace(recs, len(recs), B, C.byref(need))
            ent = self._statics[key] = dict(x=sx, cols=sc, recs=recs, B=B, ws=torch.empty(need.value, device=dev),
                                            terms=torch.empty(B, len(recs), device=dev), coef=torch.full((1,), 1.0 / B, device=dev))
        ent["x"].copy_(x, non_blocking=True)  # (device to device: _prep_x has moved the image)
        for k, v in cols.items():
            if v.shape != ent["cols"][k].shape:
                raise ValueError(f"PredictorTrainStep: observation {k!r} changed shape from {tuple(ent['cols'][k].shape)} to {tuple(v.shape)}")
            # a host column may be a temporary of _cols: only a copy that has finished may let go of it
            ent["cols"][k].copy_(v, non_blocking=v.is_cuda)
        return ent

    def _fwd_bwd(self, ent, dx=None):
        st = torch.cuda.current_stream(self.device).cuda_stream
        recs, B, ws = ent["recs"], ent["B"], ent["ws"]
        self.lib.predictor_train_fwd(recs, len(recs), B, ent["x"].data_ptr(), ws.data_ptr(), ws.numel(), BN_MOMENTUM, ent["terms"].data_ptr(),
                                     None, self.out3.data_ptr() + 4, st)
        self.lib.predictor_train_bwd(recs, len(recs), B, ent["x"].data_ptr(), ws.data_ptr(), ws.numel(), ent["coef"].data_ptr(),
                                     None if dx is None else dx.data_ptr(), st)
        torch.mul(self.out3[1:2], 1.0 / B, out=self.res[0:1])

    def _optim(self):
        on, ema = self._on, self.ema_model is not None
        # EMA of the running statistics: lr = wd = 0 and a zero gradient leave the buffers as they are
        stats = [(on.flat_b.data_ptr(), self._ema.flat_b.data_ptr(), on.flat_b.numel())] if ema and on.flat_b.numel() else ()
        self.tail.run(self.hp, on.flat_p, self.flat_g, self._ema.flat_p if ema else None, self.out3,
                      torch.cuda.current_stream(self.device).cuda_stream, ema_only=stats)
        self.res[1:2].copy_(self.state[NORM:NORM + 1])

    def _fwd_bwd_optim(self, ent):
        self._fwd_bwd(ent)
        self._optim()

    def _invalidate(self):
        self._on.invalidate()
        if self.ema_model is not None:
            self._ema.invalidate()

    # -- public -------------------------------------------------------------------------------------------
    def step(self, **obs):
        """One optimiser step on a batch (``x`` and every variable the image heads score or condition on).  Returns the device
        scalars ``{"loss": mean loss, "grad_norm": norm before clipping}``; nothing is read back."""
        ent = self._static_for(obs)
        self.it += 1
        key = tuple(ent["x"].shape)
        graph = self._graphs.get(key) if self.use_graph else None
        if graph is not None:
            graph.replay()
        else:
            self._fwd_bwd_optim(ent)
            if self.use_graph:
                self._graphs[key], _ = capture(lambda: self._fwd_bwd_optim(ent))
        self._invalidate()
        out = self.res.clone()
        return {"loss": out[0], "grad_norm": out[1]}

    def loss_and_grads(self, dx=False, **obs):
        """(mean loss, {parameter name: d loss / d parameter}) of a batch; with ``dx`` also ``"x"``: d loss / d image.  Updates the
        running statistics (it IS a training forward) and nothing else."""
        ent = self._static_for(obs)
        gx = torch.empty_like(ent["x"]) if dx else None
        self._fwd_bwd(ent, gx)
        self._on.invalidate()
        on = self._on
        grads = {n: self.flat_g[o:o + p.numel()].view(p.shape).clone() for n, p, o in zip(on.names, on.params, on.p_off)}
        if dx:
            grads["x"] = gx
        return self.res[0].clone(), grads

    def state_dict(self):
        """The reference checkpoint's keys (train_pgm.py:536-545): ``model_state_dict`` / ``ema_model_state_dict`` with the
        reference's parameter names, ``optimizer_state_dict`` (flat AdamW moments in ``named_parameters`` order of the image
        heads, and the device step state)."""
        sd = {"step": self.it, "model_state_dict": {k: v.detach().clone() for k, v in self.model.state_dict().items()},
              "optimizer_state_dict": self.tail.flat_optimizer_state(self._on.names)}
        if self.ema_model is not None:
            sd["ema_model_state_dict"] = {k: v.detach().clone() for k, v in self.ema_model.state_dict().items()}
        return sd

    def load_state_dict(self, sd):
        self.model.load_state_dict(sd["model_state_dict"], strict=True)  # (copies in place: the flat views stay)
        if self.ema_model is not None and "ema_model_state_dict" in sd:
            self.ema_model.load_state_dict(sd["ema_model_state_dict"], strict=True)
        self.tail.load_flat_optimizer_state(sd["optimizer_state_dict"], self._on.names)
        self.it = int(sd.get("step", 0))
        self._invalidate()
