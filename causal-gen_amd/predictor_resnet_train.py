"""Training ChestPGM's anticausal heads (mimic) on the GPU -- stage two of the reference pipeline (``src/pgm/train_pgm.py:111-170``,
``sup_epoch`` with ``--setup sup_aux``) for ``predictor_resnet.ChestPredictor`` as one fixed launch sequence:

    [step_from: augment / gather] -> Philox state + 1 -> the 40 weight images from the live parameters (cgen_weight_prep) ->
    training forward (csrc/predictor_resnet_train.inc: the eval forward + Dropout) -> every parameter gradient of loss / B ->
    global grad-norm -> clip at ``grad_clip`` / NaN-loss skip (on device) -> fused AdamW + EMA -> step counter commit

``loss`` is ``model_anticausal``'s summed negative log-likelihood of the four heads divided by the batch size; the optimiser is
the reference's ``AdamW`` under ``LambdaLR(linear_warmup)`` with ``clip_grad_norm_`` and ``EMA`` (``step_tail.StepTail``).  No host
synchronisation inside a step; the whole step is captured into one hipGraph after an eager first step.

The 68 distinct parameters (60 of the ONE trunk, then the four ``fc`` pairs, in ``named_parameters()`` order) live in one flat f32
buffer; GroupNorm has no batch statistic, so ``B >= 1`` is allowed.  Dropout (``CustomBlock.dropout``, p = 0.2, after ``relu(bn1)``
of each block) draws from the step's own Philox state, seeded from ``torch.initial_seed()`` and moved on by one inside every step.
Deviation from the reference: it runs the trunk once per head and so draws four independent masks per step; here the trunk runs
once, with one mask.

``ChestPredictor`` itself is unchanged: its ``train()`` still leaves eval mode on, ``_heads()`` still raises, and every eval route
sees the trained weights because the step drops the predictor's cached weight images after it has written the parameters.
"""
import copy
import ctypes as C

import torch

from . import _lib
from .predictor import _prep_x
from .predictor_resnet import MAX_RES, MIN_RES, _VARS, ChestPredictor, _conv_sites
from .step_tail import NORM, Flat, HyperParams, StepTail, capture, check_warmup

N_PARAMS = 68  # 20 convs, 20 GroupNorm pairs, 4 Linear pairs


class _Flat(Flat):
    """A ChestPredictor's parameters flattened (online model or EMA copy), its weight images and their descriptor tables."""

    def __init__(self, pred, dev):
        pred.to(dev)
        self.pred = pred
        named = list(pred.named_parameters())  # (the shared trunk once, under encoder_s; then the four fc pairs)
        if len(named) != N_PARAMS:
            raise ValueError(f"ChestPredictorTrainStep: expected {N_PARAMS} distinct parameters, got {len(named)}")
        super().__init__(named, dev)
        for n, p, o in zip(self.names, self.params, self.p_off):
            if ".resnet." in n:  # gamma / beta and the gradients' destinations must be 16-byte aligned
                assert p.numel() % 4 == 0 and o % 4 == 0 and p.data_ptr() % 16 == 0, (n, p.numel(), o)
        self.sites = _conv_sites(pred.encoder_s.resnet)
        self.tables = pred._weight_tables(dev)  # (the descriptors read the parameters where they are now: views of flat_p)
        assert all(w.data_ptr() == conv.weight.data_ptr() for w, (conv, _, _) in zip(self.tables["srcs"], self.sites))

    def invalidate(self):
        """The kernels write parameters through raw pointers, which the version counters ``ChestPredictor._images`` keys its cache
        on do not see: drop the cached images so that the next eval call builds them from the new values."""
        self.pred.__dict__.pop("_rt", None)


class ChestPredictorTrainStep:
    NORM_BLOCKS = 1024

    def __init__(self, pred, lr=1e-4, wd=0.1, betas=(0.9, 0.999), eps=1e-8, grad_clip=200.0, lr_warmup_steps=1, ema_rate=0.999,
                 ema=True, ema_update_after=100, use_graph=True, p_dropout=0.2, device="cuda", columns=None):
        check_warmup(lr_warmup_steps)
        if not isinstance(pred, ChestPredictor):
            raise TypeError("ChestPredictorTrainStep trains a predictor_resnet.ChestPredictor; the CNN predictors are PredictorTrainStep's")
        if not 0.0 <= float(p_dropout) < 1.0:
            raise ValueError(f"p_dropout must lie in [0, 1), got {p_dropout}")
        if pred.input_channels != 1:
            raise ValueError(f"ChestPredictorTrainStep: input_channels must be 1, got {pred.input_channels}")
        self.lib = _lib.require_gpu()
        dev = self.device = torch.device(device)
        # (no norm threshold in sup_epoch: only a non-finite norm or a NaN loss drops the step)
        self.hp = HyperParams(float(lr), (float(betas[0]), float(betas[1])), float(eps), float(wd), float(grad_clip), float("inf"),
                              int(lr_warmup_steps), float(ema_rate), int(ema_update_after))
        self.use_graph, self.p_dropout = use_graph, float(p_dropout)
        # {variable: column of ds.pa, or (first column, width)} for step_from (cf_eval.predictor_eval's convention)
        self.columns = None if columns is None else {k: (int(v), 1) if isinstance(v, int) else (int(v[0]), int(v[1])) for k, v in columns.items()}
        self.ema_model = None
        if ema:
            self.ema_model = copy.deepcopy(pred)
            self.ema_model.requires_grad_(False)
            self._ema = _Flat(self.ema_model, dev)
        self.model = pred
        self._on = _Flat(pred, dev)
        n = self._on.flat_p.numel()
        self.flat_g = torch.zeros(n, device=dev)
        self.tail = StepTail(self.lib, n, dev, self.NORM_BLOCKS)
        self.stats = self.tail.stats  # host read of the device-side step state (one sync)
        self.m, self.v, self.state, self.partial = self.tail.m, self.tail.v, self.tail.state, self.tail.partial
        self.out3 = torch.zeros(3, device=dev)  # [-, summed loss, 0]: what cgen_clip_decide tests for NaN
        self.res = torch.zeros(2, device=dev)   # [mean loss, gradient norm] of the last step
        # Philox state {seed, offset} of Dropout and of step_from's crop / flip draws (different streams of one state)
        self._rng = torch.tensor([torch.initial_seed() & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64, device=dev)
        self._statics, self._graphs = {}, {}
        self._last = None  # (B, R) of the last forward
        self.it = 0

    # -- pieces -------------------------------------------------------------------------------------------
    def _build(self, B, R, x, at):
        """Argument record, workspace and coefficient of a batch shape reading the static image `x`.  ``at(var)`` = (address, row
        stride in floats, width) of a variable's rows."""
        dev, on, pred = self.device, self._on, self.model
        if R != pred.input_res or not MIN_RES <= R <= MAX_RES:
            raise ValueError(f"ChestPredictorTrainStep: built for square images of input_res {pred.input_res} within {MIN_RES}..{MAX_RES}, got {R}")
        g_of = {id(p): self.flat_g.data_ptr() + 4 * o for p, o in zip(on.params, on.p_off)}
        a = _lib.ResnetTrainArgs()
        a.net.res, a.net.std_fixed = R, float(pred.std_fixed)
        for i, (conv, norm, _) in enumerate(on.sites):
            a.net.img_fwd[i], a.net.img_dg[i] = on.tables["fwd"][i].data_ptr(), on.tables["dg"][i].data_ptr()
            a.net.gamma[i], a.net.beta[i] = norm.weight.data_ptr(), norm.bias.data_ptr()
            a.gw[i], a.ggamma[i], a.gbeta[i] = g_of[id(conv.weight)], g_of[id(norm.weight)], g_of[id(norm.bias)]
        for h, enc in enumerate(pred._encoders()):
            a.net.fc_w[h], a.net.fc_b[h] = enc.fc.weight.data_ptr(), enc.fc.bias.data_ptr()
            a.gfc_w[h], a.gfc_b[h] = g_of[id(enc.fc.weight)], g_of[id(enc.fc.bias)]
        for h, var in enumerate(_VARS):
            ptr, stride, width = at(var)
            if width < (3 if var == "race" else 1):
                raise ValueError(f"ChestPredictorTrainStep: observation {var!r} has {width} columns")
            a.net.obs[h], a.net.obs_stride[h] = ptr, stride
        a.net.ctx, a.net.ctx_stride, _ = at("finding")
        a.rng, a.p_dropout = self._rng.data_ptr(), self.p_dropout
        need = _lib.i64(0)
        self.lib.resnet_train_workspace(B, R, C.byref(need))
        return dict(args=a, B=B, R=R, x=x, ws=torch.empty(need.value, device=dev), terms=torch.empty(B, 4, device=dev),
                    coef=torch.full((1,), 1.0 / B, device=dev))

    def _static_for(self, obs):
        """Static input buffers, argument record and workspace of a batch shape; `obs` is copied into the buffers."""
        x = _prep_x(obs["x"])
        if x.dim() != 4 or x.shape[0] < 1 or x.shape[1] != 1 or x.shape[-1] != x.shape[-2]:
            raise ValueError(f"ChestPredictorTrainStep: needs x of [B >= 1, 1, R, R], got {tuple(x.shape)}")
        B, R = int(x.shape[0]), int(x.shape[-1])
        cols = {}
        for var in _VARS:
            if var not in obs:
                raise KeyError(f"ChestPredictorTrainStep: observation {var!r} is missing")
            cols[var] = obs[var].detach().reshape(B, -1).float()
        key = tuple(x.shape)
        ent = self._statics.get(key)
        if ent is None:
            sc = {k: torch.empty(v.shape, device=self.device) for k, v in cols.items()}
            xs = torch.empty_like(x, device=self.device)
            ent = self._statics[key] = self._build(B, R, xs, lambda var: (sc[var].data_ptr(), sc[var].shape[1], sc[var].shape[1]))
            ent["cols"] = sc
        ent["x"].copy_(x, non_blocking=True)  # (device to device: _prep_x has moved the image)
        for k, v in cols.items():
            if v.shape != ent["cols"][k].shape:
                raise ValueError(f"ChestPredictorTrainStep: observation {k!r} changed shape from {tuple(ent['cols'][k].shape)} to {tuple(v.shape)}")
            # a host column may be a temporary: only a copy that has finished may let go of it
            ent["cols"][k].copy_(v, non_blocking=v.is_cuda)
        return key, ent

    def _static_from(self, ds, index, train, draws_out):
        """Static image, parents rows and index of a (data set, batch size): the record points into the gathered parents rows."""
        if self.columns is None:
            raise ValueError("ChestPredictorTrainStep.step_from: name the columns of ds.pa at construction (columns={variable: column})")
        missing = [v for v in _VARS if v not in self.columns]
        if missing:
            raise ValueError(f"ChestPredictorTrainStep.step_from: no column was named for {missing}")
        if index.dtype != torch.int64 or index.dim() != 1 or index.device.type != "cuda":
            raise ValueError("ChestPredictorTrainStep.step_from: the index must be a device int64 vector")
        B = int(index.numel())
        if B < 1:
            raise ValueError("ChestPredictorTrainStep.step_from: an empty index")
        if draws_out is not None:
            assert draws_out.dtype == torch.int32 and tuple(draws_out.shape) == (B, 3) and draws_out.is_contiguous() and draws_out.is_cuda
        key = (ds.key(train), B, None if draws_out is None else draws_out.data_ptr())
        ent = self._statics.get(key)
        if ent is None:
            dev = self.device
            if ds.c != 1:
                raise ValueError(f"ChestPredictorTrainStep.step_from: the data set has {ds.c} channels, the predictor reads 1")
            for var in _VARS:
                c0, k = self.columns[var]
                if not 0 <= c0 <= ds.ctx - k:
                    raise ValueError(f"ChestPredictorTrainStep.step_from: variable {var!r}: columns {c0}..{c0 + k - 1} do not fit ds.pa's {ds.ctx}")
            r_h, r_w, _, _, _ = ds.geometry(train)
            if r_h != r_w:
                raise ValueError(f"ChestPredictorTrainStep.step_from: the crop is {r_h} x {r_w}, the predictor reads square images")
            x = torch.empty((B, 1, r_h, r_w), device=dev)
            pa = torch.zeros((B, ds.ctx), device=dev)
            ent = self._statics[key] = self._build(B, r_h, x, lambda var: (pa.data_ptr() + 4 * self.columns[var][0], ds.ctx, self.columns[var][1]))
            view = _lib.View(x.data_ptr(), r_h * r_w, r_w, 1, 1, 0)  # one channel: NHWC and NCHW are the same memory
            index_buf = torch.zeros(B, dtype=torch.int64, device=dev)
            args = ds.args_for(_lib.F32, B, index_buf.data_ptr(), view, self._rng.data_ptr(), train, None,
                               None if draws_out is None else draws_out.data_ptr(), pa.data_ptr())
            ent.update(pa=pa, index=index_buf, aug=args, keep=(ds, draws_out))
        ent["index"].copy_(index, non_blocking=True)
        return key, ent

    def _fwd_bwd(self, ent, dx=None):
        """Philox state + 1, [augment], the weight images, the training forward and every gradient of loss / B"""
        st = torch.cuda.current_stream(self.device).cuda_stream
        lib, a, B, ws, t = self.lib, ent["args"], ent["B"], ent["ws"], self._on.tables
        lib.rng_advance(self._rng.data_ptr(), 1, st)
        if "aug" in ent:
            lib.batch_augment(C.byref(ent["aug"]), st)
        lib.weight_prep(t["tab"].data_ptr(), t["csite"].data_ptr(), t["cidx"].data_ptr(), t["nchunks"], st)
        lib.resnet_train_fwd(C.byref(a), B, ent["x"].data_ptr(), ws.data_ptr(), ws.numel(), ent["terms"].data_ptr(), None,
                             self.out3.data_ptr() + 4, st)
        lib.resnet_train_bwd(C.byref(a), B, ent["x"].data_ptr(), ws.data_ptr(), ws.numel(), ent["coef"].data_ptr(),
                             None if dx is None else dx.data_ptr(), st)
        torch.mul(self.out3[1:2], 1.0 / B, out=self.res[0:1])

    def _optim(self):
        ema = self.ema_model is not None
        self.tail.run(self.hp, self._on.flat_p, self.flat_g, self._ema.flat_p if ema else None, self.out3,
                      torch.cuda.current_stream(self.device).cuda_stream)
        self.res[1:2].copy_(self.state[NORM:NORM + 1])

    def _fwd_bwd_optim(self, ent):
        self._fwd_bwd(ent)
        self._optim()

    def _invalidate(self):
        self._on.invalidate()
        if self.ema_model is not None:
            self._ema.invalidate()

    def _run(self, key, ent):
        self.it += 1
        self._last = ent
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
        """One optimiser step on a batch (``x`` [B >= 1, 1, R, R], ``sex``, ``race`` one-hot, ``finding``, ``age``).  Returns the
        device scalars ``{"loss": mean loss, "grad_norm": norm before clipping}``; nothing is read back."""
        return self._run(*self._static_for(obs))

    def step_from(self, ds, index, train=True, draws_out=None):
        """One optimiser step on rows ``index`` (device int64 vector) of a one-channel ``data.DeviceDataset`` whose ``pa`` holds
        the four variables in the columns named at construction.  Inside the captured step ONE augment launch writes the static
        image and gathers the parents rows, and the heads read those rows in place.  ``draws_out`` (device int32 [B, 3]) receives
        the (oy, ox, flip) used, as in ``PredictorTrainStep.step_from``."""
        return self._run(*self._static_from(ds, index, train, draws_out))

    def loss_and_grads(self, dx=False, **obs):
        """(mean loss, {parameter name: d loss / d parameter}) of a batch; with ``dx`` also ``"x"``: d loss / d image.  It IS a
        training forward: the Philox state moves on by one, as in a step, and nothing else changes."""
        _, ent = self._static_for(obs)
        gx = torch.empty_like(ent["x"]) if dx else None
        self._last = ent
        self._fwd_bwd(ent, gx)
        on = self._on
        grads = {n: self.flat_g[o:o + p.numel()].view(p.shape).clone() for n, p, o in zip(on.names, on.params, on.p_off)}
        if dx:
            grads["x"] = gx
        return self.res[0].clone(), grads

    @torch.no_grad()
    def dropout_keep(self, k):
        """The decisions Dropout took in block ``k`` of the last forward: bool [B, C, H, W], True = kept."""
        if self._last is None:
            raise RuntimeError("ChestPredictorTrainStep.dropout_keep: no forward has run yet")
        B, R = self._last["B"], self._last["R"]
        off, h, c = _lib.i64(0), _lib.i32(0), _lib.i32(0)
        self.lib.resnet_site(B, R, 1 + 2 * int(k), C.byref(off), C.byref(h), C.byref(c))
        out = torch.empty((B, h.value, h.value, c.value), dtype=torch.uint8, device=self.device)
        self.lib.resnet_dropout_keep(self._rng.data_ptr(), self.p_dropout, B, R, int(k), out.data_ptr(),
                                     torch.cuda.current_stream(self.device).cuda_stream)
        return out.permute(0, 3, 1, 2).contiguous().bool()

    @torch.no_grad()
    def trunk_activations(self):
        """f32 NCHW copies of what the last training forward left in its workspace, in ``ChestPredictor.trunk_activations``'s
        order (relu(bn1) of each block AFTER Dropout)."""
        if self._last is None:
            raise RuntimeError("ChestPredictorTrainStep.trunk_activations: no forward has run yet")
        B, R, ws = self._last["B"], self._last["R"], self._last["ws"]
        out = []
        for site in range(_lib.RESNET_SITES):
            off, h, c = _lib.i64(0), _lib.i32(0), _lib.i32(0)
            self.lib.resnet_site(B, R, site, C.byref(off), C.byref(h), C.byref(c))
            v = ws[off.value:off.value + B * h.value * h.value * c.value].view(B, h.value, h.value, c.value)
            out.append(v.permute(0, 3, 1, 2).contiguous())
        return out

    def workspace_bytes(self):
        """{batch key: bytes of its workspace}"""
        return {k: 4 * e["ws"].numel() for k, e in self._statics.items()}

    def state_dict(self):
        """The reference checkpoint's keys (train_pgm.py:536-545): ``model_state_dict`` / ``ema_model_state_dict`` with all 248
        ``encoder_*`` names, ``optimizer_state_dict`` (flat AdamW moments in ``named_parameters()`` order and the device step
        state), and the Philox state."""
        sd = {"step": self.it, "model_state_dict": {k: v.detach().clone() for k, v in self.model.state_dict().items()},
              "optimizer_state_dict": self.tail.flat_optimizer_state(self._on.names), "rng_state": self._rng.clone()}
        if self.ema_model is not None:
            sd["ema_model_state_dict"] = {k: v.detach().clone() for k, v in self.ema_model.state_dict().items()}
        return sd

    def load_state_dict(self, sd):
        self.model.load_state_dict(sd["model_state_dict"], strict=True)  # (copies in place: the flat views stay)
        if self.ema_model is not None and "ema_model_state_dict" in sd:
            self.ema_model.load_state_dict(sd["ema_model_state_dict"], strict=True)
        self.tail.load_flat_optimizer_state(sd["optimizer_state_dict"], self._on.names)
        if "rng_state" in sd:
            self._rng.copy_(sd["rng_state"])
        self.it = int(sd.get("step", 0))
        self._invalidate()
