"""Training the anticausal predictors on the GPU -- stage two of the reference pipeline (``src/pgm/train_pgm.py:111-170``,
``sup_epoch`` with ``--setup sup_aux``) as a fixed launch sequence:

    training forward (batch-statistic BatchNorm, csrc/predictor_train.inc) -> parameter gradients of loss / B ->
    global grad-norm -> clip at ``grad_clip`` / NaN-loss skip (on device) -> fused AdamW + EMA -> step counter commit

``loss`` is ``model_anticausal``'s summed negative log-likelihood of the trained heads divided by the batch size; the optimiser is
the reference's ``AdamW(lr, betas, eps, wd)`` under ``LambdaLR(linear_warmup(lr_warmup_steps))`` with ``clip_grad_norm_`` and
``EMA(beta=ema_rate)``.  The step tail is ``TrainStep``'s (csrc/optim.hip); the float buffers (the BatchNorm running statistics)
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
import copy
import ctypes as C

import torch

from . import _lib
from .predictor import CNN, _Head, _prep_x
from .step_tail import NORM, Flat, HyperParams, StepTail, capture, check_warmup, flatten

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


class PredictorTrainStep:
    NORM_BLOCKS = 1024

    def __init__(self, pred, lr=1e-4, wd=0.1, betas=(0.9, 0.999), eps=1e-8, grad_clip=200.0, lr_warmup_steps=1, ema_rate=0.999,
                 ema=True, use_graph=True, ema_update_after=100, device="cuda", scalar_heads=False, columns=None):
        check_warmup(lr_warmup_steps)
        self.lib = _lib.require_gpu()
        dev = self.device = torch.device(device)
        # (no norm threshold in sup_epoch: only a non-finite norm or a NaN loss drops the step)
        self.hp = HyperParams(float(lr), (float(betas[0]), float(betas[1])), float(eps), float(wd), float(grad_clip), float("inf"),
                              int(lr_warmup_steps), float(ema_rate), int(ema_update_after))
        self.use_graph = use_graph
        # {variable: column of ds.pa, or (first column, width)} for step_from (cf_eval.predictor_eval's convention)
        self.columns = None if columns is None else {k: (int(v), 1) if isinstance(v, int) else (int(v[0]), int(v[1])) for k, v in columns.items()}
        self.ema_model = None
        if ema:
            self.ema_model = copy.deepcopy(pred)
            self.ema_model.requires_grad_(False)
            self._ema = _Flat(self.ema_model, dev, scalar_heads)
        self.model = pred
        self._on = _Flat(pred, dev, scalar_heads)
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
        self._rng = None  # own Philox state {seed, offset} of step_from's crop / flip draws
        self.it = 0

    # -- pieces -------------------------------------------------------------------------------------------
    def _cols(self, obs, B):
        """{variable: [B, k] f32} of every observed / context variable the trained heads read"""
        out = {}
        for var in self._on.variables():
            if var not in obs:
                raise KeyError(f"PredictorTrainStep: observation {var!r} is missing")
            out[var] = obs[var].detach().reshape(B, -1).float()
        return out

    def _build(self, xshape, at, dense):
        """Head records, workspaces and coefficient of a batch shape reading the static image `x`.  ``at(var)`` = (address, row
        stride in floats, width) of a variable's rows; ``dense[var]``: the contiguous [B, k] buffer of a context variable."""
        dev, on, B = self.device, self._on, int(xshape[0])
        recs = (_lib.PredTrainHead * len(on.heads))()
        g_of = {id(p): self.flat_g.data_ptr() + 4 * o for p, o in zip(on.params, on.p_off)}
        for r, hd in zip(recs, on.heads):
            cnn = hd.cnn
            if tuple(cnn.in_shape) != tuple(xshape[1:]):
                raise ValueError(f"predictor head for {hd.var}: built for input {cnn.in_shape}, got {tuple(xshape[1:])}")
            h = r.hd
            h.c, h.res, h.width, h.nout, h.ctx = xshape[1], xshape[-1], cnn.width, cnn.num_outputs, cnn.context_dim
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
                if dense[hd.ctx_var].shape[1] != cnn.context_dim:
                    raise ValueError(f"predictor head for {hd.var}: context {hd.ctx_var} has {dense[hd.ctx_var].shape[1]} columns, "
                                     f"expected {cnn.context_dim}")
                h.y = dense[hd.ctx_var].data_ptr()
            h.obs, h.obs_stride, _ = at(hd.var)
        need = _lib.i64(0)
        self.lib.predictor_train_workspace(recs, len(recs), B, C.byref(need))
        ent = dict(recs=recs, B=B, ws=torch.empty(need.value, device=dev), terms=torch.empty(B, len(recs), device=dev),
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
        """Static input buffers, head records, workspace and coefficient of a batch shape; `obs` is copied into the buffers."""
        x = _prep_x(obs["x"])
        B = int(x.shape[0])
        if B < 2:
            raise ValueError("PredictorTrainStep: train-mode BatchNorm needs a batch of at least 2 images")
        cols = self._cols(obs, B)
        key = tuple(x.shape)
        ent = self._statics.get(key)
        if ent is None:
            sc = {k: torch.empty(v.shape, device=self.device) for k, v in cols.items()}
            ent = self._statics[key] = self._build(x.shape, lambda var: (sc[var].data_ptr(), sc[var].shape[1], sc[var].shape[1]), sc)
            ent.update(x=torch.empty_like(x, device=self.device), cols=sc)
        ent["x"].copy_(x, non_blocking=True)  # (device to device: _prep_x has moved the image)
        for k, v in cols.items():
            if v.shape != ent["cols"][k].shape:
                raise ValueError(f"PredictorTrainStep: observation {k!r} changed shape from {tuple(ent['cols'][k].shape)} to {tuple(v.shape)}")
            # a host column may be a temporary of _cols: only a copy that has finished may let go of it
            ent["cols"][k].copy_(v, non_blocking=v.is_cuda)
        return ent

    def _static_from(self, ds, index, train, draws_out):
        """Static image, parents rows and index of a (data set, batch size): the head records point into the gathered parents rows
        wherever a row stride is allowed (obs, the scalar heads' inputs); a context is copied out densely inside the step."""
        if self.columns is None:
            raise ValueError("PredictorTrainStep.step_from: name the columns of ds.pa at construction (columns={variable: column})")
        missing = [v for v in self._on.variables() if v not in self.columns]
        if missing:
            raise ValueError(f"PredictorTrainStep.step_from: no column was named for {missing}")
        if index.dtype != torch.int64 or index.dim() != 1 or index.device.type != "cuda":
            raise ValueError("PredictorTrainStep.step_from: the index must be a device int64 vector")
        B = int(index.numel())
        if B < 2:
            raise ValueError("PredictorTrainStep: train-mode BatchNorm needs a batch of at least 2 images")
        if draws_out is not None:
            assert draws_out.dtype == torch.int32 and tuple(draws_out.shape) == (B, 3) and draws_out.is_contiguous() and draws_out.is_cuda
        key = (ds.key(train), B, None if draws_out is None else draws_out.data_ptr())
        ent = self._statics.get(key)
        if ent is None:
            dev = self.device
            for var in self._on.variables():
                c0, k = self.columns[var]
                if not 0 <= c0 <= ds.ctx - k:
                    raise ValueError(f"PredictorTrainStep.step_from: variable {var!r}: columns {c0}..{c0 + k - 1} do not fit ds.pa's {ds.ctx}")
            r_h, r_w, _, _, _ = ds.geometry(train)
            x = torch.empty((B, ds.c, r_h, r_w), device=dev)
            pa = torch.zeros((B, ds.ctx), device=dev)
            ctx_vars = list(dict.fromkeys(hd.ctx_var for hd in self._on.heads if hd.ctx_var is not None))
            dense = {v: torch.empty((B, self.columns[v][1]), device=dev) for v in ctx_vars}
            ent = self._statics[key] = self._build(x.shape, lambda var: (pa.data_ptr() + 4 * self.columns[var][0], ds.ctx, self.columns[var][1]), dense)
            if self._rng is None:
                self._rng = torch.tensor([torch.initial_seed() & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64, device=dev)
            # one channel: NHWC and planar are the same memory and the existing launch serves; else the planar one
            view = _lib.View(x.data_ptr(), r_h * r_w, r_w, 1, 1, 0) if ds.c == 1 else ds.planar_view(x.data_ptr(), train)
            index_buf = torch.zeros(B, dtype=torch.int64, device=dev)
            args = ds.args_for(_lib.F32, B, index_buf.data_ptr(), view, self._rng.data_ptr(), train, None,
                               None if draws_out is None else draws_out.data_ptr(), pa.data_ptr())
            ent.update(x=x, pa=pa, index=index_buf, aug=args, train=train, planar=ds.c != 1, keep=(ds, draws_out),
                       gather=[(dense[v], pa[:, self.columns[v][0]:self.columns[v][0] + self.columns[v][1]]) for v in ctx_vars])
        ent["index"].copy_(index, non_blocking=True)
        return key, ent

    def _load(self, ent):
        """step_from's batch, inside the step: the next crop / flip draws, one augment launch into the static image with the
        parents rows gathered on the side, and the dense copies of the context columns"""
        st = torch.cuda.current_stream(self.device).cuda_stream
        if ent["train"]:
            self.lib.rng_advance(self._rng.data_ptr(), 1, st)
        (self.lib.batch_augment_planar if ent["planar"] else self.lib.batch_augment)(C.byref(ent["aug"]), st)
        for dst, src in ent["gather"]:
            dst.copy_(src)

    def _fwd_bwd(self, ent, dx=None):
        st = torch.cuda.current_stream(self.device).cuda_stream
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

    def _optim(self):
        on, ema = self._on, self.ema_model is not None
        # EMA of the running statistics: lr = wd = 0 and a zero gradient leave the buffers as they are
        stats = [(on.flat_b.data_ptr(), self._ema.flat_b.data_ptr(), on.flat_b.numel())] if ema and on.flat_b.numel() else ()
        self.tail.run(self.hp, on.flat_p, self.flat_g, self._ema.flat_p if ema else None, self.out3,
                      torch.cuda.current_stream(self.device).cuda_stream, ema_only=stats)
        self.res[1:2].copy_(self.state[NORM:NORM + 1])

    def _fwd_bwd_optim(self, ent):
        if "aug" in ent:
            self._load(ent)
        self._fwd_bwd(ent)
        self._optim()

    def _invalidate(self):
        self._on.invalidate()
        if self.ema_model is not None:
            self._ema.invalidate()

    def _run(self, key, ent):
        self.it += 1
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

    # -- public -------------------------------------------------------------------------------------------
    def step(self, **obs):
        """One optimiser step on a batch (``x`` and every variable the trained heads score or condition on; with ``scalar_heads``
        that includes ``age``).  Returns the device scalars ``{"loss": mean loss, "grad_norm": norm before clipping}``; nothing
        is read back."""
        ent = self._static_for(obs)
        return self._run(tuple(ent["x"].shape), ent)

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
        reference's parameter names, ``optimizer_state_dict`` (flat AdamW moments in ``named_parameters`` order of the trained
        heads -- image heads, then scalar heads -- and the device step state)."""
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
