"""Training ChestPGM's anticausal heads (mimic) on the GPU -- stage two of the reference pipeline (``src/pgm/train_pgm.py:111-170``,
``sup_epoch`` with ``--setup sup_aux``) for ``predictor_resnet.ChestPredictor`` as one fixed launch sequence:

    [step_from: augment / gather] -> Philox state + 1 -> the 40 weight images from the live parameters (cgen_weight_prep) ->
    training forward (csrc/predictor_resnet_train.inc: the eval forward + Dropout) -> every parameter gradient of loss / B ->
    global grad-norm -> clip at ``grad_clip`` / NaN-loss skip (on device) -> fused AdamW + EMA -> step counter commit

``loss`` is ``model_anticausal``'s summed negative log-likelihood of the four heads divided by the batch size; the optimiser is
the reference's ``AdamW`` under ``LambdaLR(linear_warmup)`` with ``clip_grad_norm_`` and ``EMA`` (``step_tail.StepTail``; the
skeleton around it, the staging of ``step`` and the data-set half of ``step_from`` are ``step_tail.ImageSupStep``'s).  No host
synchronisation inside a step; the whole step is captured into one hipGraph after an eager first step.

The 68 distinct parameters (60 of the ONE trunk, then the four ``fc`` pairs, in ``named_parameters()`` order) live in one flat f32
buffer; GroupNorm has no batch statistic, so ``B >= 1`` is allowed.  Dropout (``CustomBlock.dropout``, p = 0.2, after ``relu(bn1)``
of each block) draws from the step's own Philox state, seeded from ``torch.initial_seed()`` and moved on by one inside every step.
Deviation from the reference: it runs the trunk once per head and so draws four independent masks per step; here the trunk runs
once, with one mask.

``ChestPredictor`` itself is unchanged: its ``train()`` still leaves eval mode on, ``_heads()`` still raises, and every eval route
sees the trained weights because the step drops the predictor's cached weight images after it has written the parameters.
"""
import ctypes as C

import torch

from . import _lib
from .predictor import _prep_x
from .predictor_resnet import MAX_RES, MIN_RES, _VARS, ChestPredictor, _conv_sites
from .step_tail import Flat, ImageSupStep

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


class ChestPredictorTrainStep(ImageSupStep):
    """``state_dict()`` holds all 248 ``encoder_*`` names, the optimiser state in ``named_parameters()`` order, and the Philox state
    (``rng_state``)."""
    NORM_BLOCKS = 1024

    def __init__(self, pred, lr=1e-4, wd=0.1, betas=(0.9, 0.999), eps=1e-8, grad_clip=200.0, lr_warmup_steps=1, ema_rate=0.999,
                 ema=True, ema_update_after=100, use_graph=True, p_dropout=0.2, device="cuda", columns=None):
        if not isinstance(pred, ChestPredictor):
            raise TypeError("ChestPredictorTrainStep trains a predictor_resnet.ChestPredictor; the CNN predictors are PredictorTrainStep's")
        if not 0.0 <= float(p_dropout) < 1.0:
            raise ValueError(f"p_dropout must lie in [0, 1), got {p_dropout}")
        if pred.input_channels != 1:
            raise ValueError(f"ChestPredictorTrainStep: input_channels must be 1, got {pred.input_channels}")
        super().__init__(pred, columns, lr=lr, wd=wd, betas=betas, eps=eps, grad_clip=grad_clip, lr_warmup_steps=lr_warmup_steps,
                         ema_rate=ema_rate, ema=ema, use_graph=use_graph, ema_update_after=ema_update_after, device=device)
        self.p_dropout = float(p_dropout)
        # Philox state {seed, offset} of Dropout and of step_from's crop / flip draws (different streams of one state)
        self._rng = self._new_rng()
        self._last = None  # the entry of the last forward

    # -- pieces -------------------------------------------------------------------------------------------
    def _flatten(self, pred, dev):
        return _Flat(pred, dev)

    def _variables(self):
        return _VARS

    def _check_batch(self, B):
        if B < 1:
            raise ValueError("ChestPredictorTrainStep.step_from: an empty index")

    def _check_geometry(self, ds, r_h, r_w):
        if ds.c != 1:
            raise ValueError(f"ChestPredictorTrainStep.step_from: the data set has {ds.c} channels, the predictor reads 1")
        if r_h != r_w:
            raise ValueError(f"ChestPredictorTrainStep.step_from: the crop is {r_h} x {r_w}, the predictor reads square images")

    def _build(self, x, at, dense):
        """Argument record, workspace and coefficient of a batch shape reading the static image `x`.  ``at(var)`` = (address, row
        stride in floats, width) of a variable's rows (``finding`` is read where it lies: no `dense` copy)."""
        dev, on, pred, B, R = self.device, self._on, self.model, int(x.shape[0]), int(x.shape[-1])
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
        x = _prep_x(obs["x"])
        if x.dim() != 4 or x.shape[0] < 1 or x.shape[1] != 1 or x.shape[-1] != x.shape[-2]:
            raise ValueError(f"ChestPredictorTrainStep: needs x of [B >= 1, 1, R, R], got {tuple(x.shape)}")
        return self._stage(x, obs)

    def _fwd_bwd(self, ent, dx=None):
        """Philox state + 1, [augment], the weight images, the training forward and every gradient of loss / B"""
        st = self._stream()
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

    def _run(self, key, ent):
        self._last = ent
        return super()._run(key, ent)

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
        grads = self._grads()
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

    def _extra_state(self):
        return {"rng_state": self._rng.clone()}

    def _load_extra_state(self, sd):
        if "rng_state" in sd:
            self._rng.copy_(sd["rng_state"])
