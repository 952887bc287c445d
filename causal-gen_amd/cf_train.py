"""Counterfactual fine-tuning on the GPU -- the ``is_train`` branch of ``cf_epoch`` (``src/pgm/train_cf.py:140-180``) as a fixed launch
sequence without a host read:

    [step_from: the Gumbel-max uniforms of the PGM, if it has such a mechanism (cgen_philox_uniform on the engine's Philox state) ->
    counterfactual parents (cgen_pgm_counterfactual)] -> rng advance -> factual ELBO, abduction and counterfactual replay
    on one tape (HVAE._run_dscm_forward; step_from: the augment launch is its first) -> anticausal predictor forward on cf_x ->
    non-finite counts of the head outputs x2 -> the Lagrangian (cgen_cf_lagrange) -> predictor input gradient at 1 / B ->
    d cf_x / d head outputs -> ELBO seeds -> engine backward -> global grad-norm with the multiplier's slot -> clip / skip ->
    fused AdamW + EMA at a constant lr -> the multiplier's AdamW(maximize), clamp and EMA (cgen_lagrange_step) -> step commit

``loss = aux_loss - (lmbda - damping sg(eps - elbo)) (eps - elbo)`` (dscm.py:78-88).  The reference drops a step whose loss is NaN
(dscm.py:75 ``check_nan``, train_cf.py:161-164); here the non-finite counts of the abduction's and the replay's head outputs and the
loss itself set a NaN gate that ``cgen_clip_decide`` turns into the skip flag.  The per-step ``.item()`` bookkeeping of
train_cf.py:205-210 is a block of running sums on the device, read once per epoch (``epoch_stats``).

f32 engine, one particle, one GPU; ``DSCM.forward`` and its autograd path are untouched and remain the host composition this replaces.

The predictor sits behind one seam (``cf_heads``): its variables, its records for a static batch, a forward that writes per-sample
terms and their sum, a backward that writes ``d aux / d cf_x`` at the device coefficient 1 / B.  ``CnnHeads`` serves the predictors of
``predictor.make_predictor`` (morphomnist, cmnist, ukbb: the launches the step always had), ``ChestHeads`` mimic's
``predictor_resnet.ChestPredictor`` (one trunk, four heads, ``terms`` [B, 4], the observations read in place at their strides).

Device buffers (all f32 unless said):
  ``lag``  [4] = {lmbda, exp_avg, exp_avg_sq, EMA of lmbda}; ``dscm.lmbda.data`` is ``lag[0:1]``, ``ema_model.lmbda.data`` is ``lag[3:4]``
  ``res``  [4] = {loss, aux_loss, d loss / d lmbda, w = d loss / d elbo}          (cgen_cf_lagrange)
  ``coef`` [3] = {w S / (B dims), w beta S / (B dims), beta}                        (TrainStep.coef's layout: the engine's seeds)
  ``gate`` [3] = {loss, NaN if the step is bad else nll, kl}                        (cgen_clip_decide's out3)
  ``sums`` [8] = {loss, aux_loss, elbo, nll, kl, n, n_bad, -}                       (running sums over the steps that are not bad)
  ``nonfinite`` int32 [2 x NONFINITE_BLOCKS]: per-block counts of the abduction's, then the replay's head outputs
  the tail's ``partial`` has ``NORM_BLOCKS + 1`` entries: the last is the multiplier's squared gradient
"""
import copy
import ctypes as C
import random

import torch

from . import _lib
from .cf_heads import heads_for, kind_of
from .engine import StaticParents, compact_parents
from .step_tail import (STATE_FLOATS, HyperParams, StepTail, capture, check_index, mark_weights_written, normalize_columns, pin_drop_cond,
                        ranges_where)

LMBDA, LM, LV, LEMA = range(4)
S_LOSS, S_AUX, S_ELBO, S_NLL, S_KL, S_N, S_BAD = range(7)


def _check(dscm, args, lr, lr_lagrange, process_group):
    """Everything CfTrainStep refuses, before any device work."""
    vae = dscm.vae
    if getattr(vae, "compute_dtype", "f32") != "f32":
        raise ValueError(f"CfTrainStep: the HVAE's compute_dtype is {vae.compute_dtype!r}; 16-bit fine-tuning is not validated (the "
                         "differentiable DSCM path has only been held to its reference on the f32 engine)")
    particles = int(getattr(args, "cf_particles", 1) or 1)
    if particles != 1:
        raise ValueError(f"CfTrainStep: cf_particles = {particles}; one particle per step is served")
    if process_group is not None:
        raise ValueError("CfTrainStep: data parallelism is not served (no process group)")
    lk = getattr(vae, "likelihood", None)
    if not getattr(vae, "_dscm_differentiable", False) or getattr(lk, "kind", None) not in ("dgauss", "dmol") or getattr(lk, "logit_space", False):
        raise ValueError("CfTrainStep: the differentiable counterfactual step is built for the DGaussNet and DmolNet heads of vae.HVAE; "
                         f"{type(vae).__name__} with {type(lk).__name__} has none")
    if not (float(lr) > 0.0 and float(lr_lagrange) > 0.0):
        raise ValueError(f"CfTrainStep: learning rates must be positive (lr = {lr}, lr_lagrange = {lr_lagrange})")
    if dscm.predictor is None or kind_of(dscm.predictor) is None:
        raise ValueError("CfTrainStep: the predictor must be one of predictor.make_predictor's (CNN heads) or a "
                         f"predictor_resnet.ChestPredictor; {type(dscm.predictor).__name__} is neither")


class CfTrainStep:
    NORM_BLOCKS = 1024
    NONFINITE_BLOCKS = 64
    EMA_UPDATE_AFTER = 100  # utils.EMA's update_after_step, as TrainStep

    def __init__(self, dscm, args, lr=1e-4, lr_lagrange=1e-2, ema=True, use_graph=True, columns=None, device="cuda", process_group=None):
        _check(dscm, args, lr, lr_lagrange, process_group)
        self.lib = _lib.require_gpu()
        self.dscm, self.args, self.use_graph = dscm, args, use_graph
        self.lr, self.lr_lagrange = float(lr), float(lr_lagrange)
        self.columns = normalize_columns(columns)
        dev = torch.device(device)
        self.vae, self.pred = dscm.vae.to(dev), dscm.predictor.to(dev)
        self.eng = eng = self.vae.engine()
        dev = self.device = eng.device
        self.heads = heads_for(self.pred, dev)
        n = eng.flat_p.numel()
        self.tail = StepTail(self.lib, n, dev, self.NORM_BLOCKS, extra_norm_slots=1)
        self.state = self.tail.state
        self.beta, self.t_abduct = float(args.beta), 1.0
        self.eps, self.damping = float(args.elbo_constraint), float(args.damping)
        lm0 = float(dscm.lmbda.detach().reshape(-1)[0])
        self.lag = torch.tensor([lm0, 0.0, 0.0, lm0], device=dev)
        dscm.lmbda.data = self.lag[LMBDA:LMBDA + 1]  # the live parameter IS the device float the kernels write
        dscm.eps = dscm.eps.to(dev)
        self.res = torch.zeros(4, device=dev)
        self.coef = torch.tensor([0.0, 0.0, self.beta], device=dev)
        self.gate = torch.zeros(3, device=dev)
        self.sums = torch.zeros(8, device=dev)
        self.nonfinite = torch.zeros(2 * self.NONFINITE_BLOCKS, dtype=torch.int32, device=dev)
        self.ema_model = self.ema_vae = self.ema_flat = None
        if ema:
            from .dscm import DSCM

            self.ema_vae = copy.deepcopy(self.vae).to(dev)
            self.ema_vae.requires_grad_(False)
            self.ema_vae.eval()
            self.ema_flat = self.ema_vae.engine().flat_p
            em = self.ema_model = DSCM(dscm.args, None, None, self.ema_vae)
            em.pgm, em.predictor = dscm.pgm, dscm.predictor  # frozen, shared
            em.lmbda.requires_grad_(False)
            em.lmbda.data = self.lag[LEMA:LEMA + 1]
            em.eps = dscm.eps
        self.ranges = None
        self._ents, self._inputs, self._cfm = {}, {}, {}
        self.it = 0

    # -- pieces -----------------------------------------------------------------------------------------
    def _hp(self):
        a = self.args
        return HyperParams(self.lr, (float(a.betas[0]), float(a.betas[1])), 1e-8, float(a.wd), float(a.grad_clip), float(a.grad_skip), 1,
                           float(a.ema_rate), self.EMA_UPDATE_AFTER, True)

    def _pred_vars(self):
        """(variables the image heads score, their context variables, every variable the predictor reads), in first-use order"""
        h = self.heads
        return h.scored, h.ctx, h.every

    def _finish_entry(self, ent, xshape, at, dense, obs_views):
        """The predictor's records for a static batch (``at(var)`` = (address, row stride in floats) of a variable's rows,
        ``dense[var]`` the contiguous [B, k] buffer of a context variable) and the buffers its launches write."""
        B = int(xshape[0])
        ent.update(B=B, xshape=tuple(xshape), plan=self.heads.build(B, xshape, at, dense),
                   terms=torch.zeros(B, self.heads.n_terms, device=self.device), loss=torch.zeros(1, device=self.device),
                   inv_b=torch.full((1,), 1.0 / B, device=self.device), obs_views=obs_views, graph=None, out3=None)
        return ent

    def _static_for(self, x, pa, cf_pa, cf_obs):
        """Static copies of a batch (image, both parents, the predictor's variables) with the head records that read them."""
        B = int(x.shape[0])
        _, _, every = self._pred_vars()
        missing = [v for v in every if v not in cf_obs]
        if missing:
            raise KeyError(f"CfTrainStep.step: cf_obs lacks {missing}")
        cols = {v: cf_obs[v].detach().reshape(B, -1).float() for v in every}
        key = ("step", tuple(x.shape), x.dtype, tuple(pa.shape), compact_parents(pa) is not None, tuple(cf_pa.shape),
               compact_parents(cf_pa) is not None, tuple((v, c.shape[1]) for v, c in cols.items())) + self._drop_key()
        ent = self._ents.get(key)
        if ent is None:
            dev = self.device
            sc = {v: torch.empty(c.shape, device=dev) for v, c in cols.items()}
            ent = dict(x=x.to(dev).clone(), spa=StaticParents(pa.to(dev)), scf=StaticParents(cf_pa.to(dev)), cols=sc)
            ent["pa"], ent["cf_pa"] = ent["spa"].t, ent["scf"].t
            self._ents[key] = self._finish_entry(ent, x.shape, lambda var: (sc[var].data_ptr(), sc[var].shape[1]), sc, sc)
        else:
            ent["x"].copy_(x, non_blocking=True)
            ent["spa"].load(pa.to(self.device))
            ent["scf"].load(cf_pa.to(self.device))
        for v, c in cols.items():
            ent["cols"][v].copy_(c, non_blocking=c.is_cuda)
        return ent

    def _drop_key(self):
        """cond_prior in train mode draws ``drop_cond`` on the host: the outcome is pinned for this step and keys its graph."""
        m = self.vae
        if not (m.cond_prior and m.training):
            return ((1, 1),)
        return (pin_drop_cond(m),)

    def _pgm_cf(self, ds):
        """The counterfactual launch over ``ds.pa`` (one per table width)."""
        from .pgm_cf import DevicePGM, PgmCounterfactual
        from .pgm_train import default_columns

        cfm = self._cfm.get(ds.ctx)
        if cfm is None:
            pgm = self.dscm.pgm
            if isinstance(pgm, DevicePGM):
                if self.columns is None and pgm.cf.ncol == ds.ctx and pgm.cf.pre:
                    cfm = pgm.cf
                pgm = pgm.pgm
            if cfm is None:
                if not hasattr(pgm, "mechanisms"):
                    raise ValueError("CfTrainStep.step_from: dscm.pgm must be a DevicePGM or a PGM that DevicePGM can wrap")
                cols = default_columns(pgm)[0] if self.columns is None else {k: v[0] for k, v in self.columns.items()}
                a = self.args if getattr(self.args, "parents_x", None) else self.dscm.args
                cfm = PgmCounterfactual(pgm, a, cols, ds.ctx, device=self.device)
            if cfm.ctx != self.vae.context_dim:
                raise ValueError(f"CfTrainStep.step_from: args.parents_x gives {cfm.ctx} parent columns, the HVAE takes {self.vae.context_dim}")
            self._cfm[ds.ctx] = cfm
        return cfm

    def _static_from(self, ds, index, train):
        from .data import AugmentedInput

        check_index(index, "CfTrainStep.step_from")
        B = int(index.numel())
        key = ("from", ds.key(train), B) + self._drop_key()
        ent = self._ents.get(key)
        if ent is None:
            dev = self.device
            cfm = self._pgm_cf(ds)
            scored, ctx_vars, every = self._pred_vars()
            missing = [v for v in every if v not in cfm.columns]
            if missing:
                raise ValueError(f"CfTrainStep.step_from: no column was named for {missing}")
            width = lambda v: cfm.width.get(v, 1) if self.columns is None or v not in self.columns else self.columns[v][1]  # noqa: E731
            hook = AugmentedInput(ds, B, train)
            cf = cfm._entry(B)["cf"]  # the counterfactual table's static buffer: the heads read its columns in place
            view = lambda v: cf[:, cfm.columns[v]:cfm.columns[v] + width(v)]  # noqa: E731
            dense = {v: torch.empty((B, width(v)), device=dev) for v in ctx_vars}
            ent = dict(x=hook, cfm=cfm, ds=ds, do_index=torch.zeros(B, dtype=torch.int64, device=dev),
                       mask=torch.zeros(1, dtype=torch.int32, device=dev), gather=[(dense[v], view(v)) for v in ctx_vars])
            self._ents[key] = self._finish_entry(ent, hook.shape, lambda var: (cf.data_ptr() + 4 * cfm.columns[var], cfm.ncol), dense,
                                                 {v: view(v) for v in every})
        ent["x"].load(index)
        return ent

    def _counterfactual_parents(self, ent):
        """step_from, inside the step: one launch for the counterfactual table and both compact parents, then the dense copies of
        the predictor's context columns"""
        ds, cfm = ent["ds"], ent["cfm"]
        self.eng.rng_ptr()  # (creates the Philox state on first use; the launch below reads it, the step's advance follows)
        _, ent["pa"], ent["cf_pa"] = cfm.run(ds.pa, ent["x"].index_buf, ds.pa, ent["do_index"], do_mask_dev=ent["mask"], rng=self.eng.rng)
        for dst, src in ent["gather"]:
            dst.copy_(src)

    def _fwd_bwd(self, ent):
        """Forward, the Lagrangian and the backward pass of one static batch.  Returns the device tensor [elbo, nll, kl]."""
        m, eng, lib = self.vae, self.eng, self.lib
        B = ent["B"]
        m.__dict__["_beta_dev"] = self.coef.data_ptr() + 8
        try:
            out3, cf_x, _ = m._run_dscm_forward(ent["x"], ent["pa"], [ent["cf_pa"]], self.beta, self.t_abduct)
        finally:
            m.__dict__["_beta_dev"] = None
        st = eng.stream
        self.heads.forward(ent["plan"], cf_x, ent["terms"], ent["loss"])
        host = ent["host"] = self.heads.scalar_nll(ent["obs_views"], B)  # heads that see no image (UKBB's age): a device scalar, no gradient
        (rec_params, cf_params), = m.__dict__["_saved_cf"][0]
        nb = self.NONFINITE_BLOCKS
        for i, t in enumerate((rec_params, cf_params)):
            lib.nonfinite_partial(eng.dt, t.n, t.h, t.w, t.cv(), self.nonfinite.data_ptr() + 4 * nb * i, nb, st)
        params, xin, _, R, Cx, dims = m.__dict__["_saved"]
        S = eng.set_loss_scale(B * dims)
        q = _lib.CfLagrangeArgs()
        q.out3, q.aux_sum, q.aux_add = out3.data_ptr(), ent["loss"].data_ptr(), None if host is None else host.data_ptr()
        q.lmbda, q.beta_dev = self.lag.data_ptr() + 4 * LMBDA, self.coef.data_ptr() + 8
        q.nonfinite, q.n_nonfinite = self.nonfinite.data_ptr(), 2 * nb
        q.inv_b, q.eps, q.damping, q.seed_scale, q.beta = 1.0 / B, self.eps, self.damping, S / (B * dims), self.beta
        q.res, q.coef, q.gsq_slot, q.gate, q.sums = (self.res.data_ptr(), self.coef.data_ptr(), self.tail.extra_slot(0), self.gate.data_ptr(),
                                                     self.sums.data_ptr())
        lib.cf_lagrange(C.byref(q), st)
        # d aux_loss / d cf_x, then through cf_x = clamp(cf_loc + cf_scale (x - rec_loc) / rec_scale) into the head gradients
        dx = torch.empty_like(cf_x)
        self.heads.backward(ent["plan"], cf_x, ent["inv_b"], dx)
        g_rec, g_cfp = eng.seed_grad(rec_params), eng.seed_grad(cf_params)
        if m.likelihood.kind == "dgauss":
            eng.lib.cf_dgauss_bwd(eng.dt, B, R, R, Cx, rec_params.cv(), cf_params.cv(), xin.cv(), dx.data_ptr(), S, g_rec.cv(), g_cfp.cv(), st)
        else:
            eng.lib.cf_dmol_bwd(eng.dt, B, R, R, m._dmol_mode(True), rec_params.cv(), cf_params.cv(), xin.cv(), dx.data_ptr(), S, g_rec.cv(),
                                g_cfp.cv(), st)
        eng.launches += 1
        ent["dx"], ent["cf_x"] = dx, cf_x
        # the factual ELBO's seeds, read by the kernels from `coef` (what cgen_cf_lagrange just wrote)
        eng.kl_coef_ptr = self.coef.data_ptr() + 4
        eng.like_coef_ptr = self.coef.data_ptr()
        if not m.__dict__.get("_like_fused", False):  # (fused: the head's tape entry runs the NLL's backward itself)
            gparams = eng.seed_grad(params)
            if m.likelihood.kind == "dgauss":
                eng.lib.dgauss_nll_bwd(eng.dt, B, R, R, Cx, params.cv(), xin.cv(), self.coef.data_ptr(), 0, gparams.cv(), st)
            else:
                eng.lib.dmol_nll_bwd(eng.dt, B, R, R, params.cv(), xin.cv(), self.coef.data_ptr(), 0, gparams.cv(), st)
            eng.launches += 1
        eng.backward()
        return out3

    def _lagrange_step(self, stream):
        a = self.args
        q = _lib.LagrangeStepArgs()
        p = self.lag.data_ptr()
        q.lmbda, q.m, q.v, q.ema = p + 4 * LMBDA, p + 4 * LM, p + 4 * LV, None if self.ema_model is None else p + 4 * LEMA
        q.g, q.state_dev = self.res.data_ptr() + 8, self.state.data_ptr()
        q.lr, q.beta1, q.beta2, q.eps, q.ema_beta = self.lr_lagrange, float(a.betas[0]), float(a.betas[1]), 1e-8, float(a.ema_rate)
        q.ema_update_after = self.EMA_UPDATE_AFTER
        self.lib.lagrange_step(C.byref(q), stream)

    def _optim(self):
        eng = self.eng
        eng.stream = torch.cuda.current_stream(eng.device).cuda_stream
        if self.ranges is None:  # the parameters the backward pass writes a gradient for: the others keep weights and moments
            self.ranges = ranges_where(eng, lambda p: id(p) in eng.pgrad_init and p.requires_grad)
        self.tail.run(self._hp(), eng.flat_p, eng.flat_g, self.ema_flat, self.gate, eng.stream, ranges=self.ranges,
                      before_commit=self._lagrange_step)

    def _body(self, ent):
        if "cfm" in ent:
            self._counterfactual_parents(ent)
        out3 = self._fwd_bwd(ent)
        self._optim()
        return out3

    def _mark_weights_written(self):
        mark_weights_written(self.vae, self.ema_vae)

    def _run(self, ent):
        self.it += 1
        if ent["graph"] is not None:
            ent["graph"].replay()
            self.heads.replayed(ent["plan"])
        else:
            ent["out3"] = eager = self._body(ent)
            if self.use_graph:
                # the eager step above has moved the weights, the multiplier and the sums; the capture itself runs nothing, so the
                # graph's static [elbo, nll, kl] is unwritten until the first replay: this call's values are copied into it
                ent["graph"], ent["out3"] = capture(lambda: self._body(ent))
                ent["out3"].copy_(eager)
        self._mark_weights_written()
        return self._out(ent["out3"])

    def _out(self, out3):
        return {"loss": self.res[0], "aux_loss": self.res[1], "elbo": out3[0], "nll": out3[1], "kl": out3[2], "out3": out3}

    # -- public -------------------------------------------------------------------------------------------
    def step(self, x, pa, cf_pa, cf_obs):
        """One fine-tuning step on a batch with the caller's counterfactual parents.  `pa` / `cf_pa`: what ``vae_preprocess``
        returns, or compact ``[B, ctx]``; `cf_obs`: {variable: [B, k]} of every variable the predictor reads, under the
        intervention.  Returns device scalars (views of static buffers, valid until the next step): loss, aux_loss, elbo, nll, kl
        and ``out3``.  Nothing is read back."""
        return self._run(self._static_for(x, pa, cf_pa, cf_obs))

    def graph_count(self):
        return sum(1 for e in self._ents.values() if e["graph"] is not None)

    def step_from(self, ds, index, do_index=None, do_var=None, train=True):
        """One fine-tuning step on rows `index` (device int64 vector) of a ``data.DeviceDataset`` whose ``pa`` holds every PGM
        variable (``columns=`` at construction, default: side by side in ``pgm.variables`` order).  The intervention takes the
        value of `do_var` (default ``args.do_pa``, else a random variable of the PGM) from rows `do_index` of the same table
        (default ``index[randperm(B)]``, train_cf.py:149).  The index, the permutation and the intervention's mask word are
        copied into static buffers: another `do_var` is another mask word for the same graph.  A Gumbel-max mechanism (ChestPGM's
        ``finding | age``) takes its uniforms from the engine's Philox state (``PgmCounterfactual.run(rng=)``), read before the
        step's advance on stream ids nothing else uses, so they are this step's alone and resume with ``state_dict()``.  (With an
        injected ``vae.noise`` the engine does not advance and the uniforms repeat from step to step: tests only.)"""
        ent = self._static_from(ds, index, train)
        B = ent["B"]
        if do_index is None:
            do_index = index[torch.randperm(B, device=index.device)]
        if do_index.dtype != torch.int64 or do_index.numel() != B or do_index.device.type != "cuda":
            raise ValueError("CfTrainStep.step_from: do_index must be a device int64 vector as long as the index")
        if do_var is None:
            do_var = getattr(self.args, "do_pa", None) or random.choice(list(ent["cfm"].vars))
        ent["do_index"].copy_(do_index.reshape(-1), non_blocking=True)
        ent["mask"].fill_(ent["cfm"].mask_of([do_var] if isinstance(do_var, str) else do_var))
        return self._run(ent)

    def loss_and_grads(self, x, pa, cf_pa, cf_obs):
        """(loss, aux_loss, out3, d loss / d lmbda, {parameter name: d loss / d parameter}) of a batch -- no optimiser step, the
        running sums are left as they were."""
        ent = self._static_for(x, pa, cf_pa, cf_obs)
        sums = self.sums.clone()
        out3 = self._fwd_bwd(ent)
        self.sums.copy_(sums)
        eng = self.eng
        grads = {n: eng.param_grad_view(p).clone() for n, p in self.vae.named_parameters() if id(p) in eng.pgrad_init}
        return self.res[0].clone(), self.res[1].clone(), out3.clone(), self.res[2].clone(), grads

    def stats(self):
        """The tail's statistics plus the multiplier and the number of bad (non-finite) steps: one copy to the host, one sync."""
        s = torch.cat([self.state, self.lag[LMBDA:LMBDA + 1], self.sums[S_BAD:S_BAD + 1]]).cpu().tolist()
        out = StepTail.stats_of(s[:STATE_FLOATS])
        out.update(lmbda=s[STATE_FLOATS], n_bad=int(s[STATE_FLOATS + 1]))
        return out

    def epoch_stats(self, reset=True):
        """Means of loss, aux_loss, elbo, nll and kl over the steps since the last reset that were not bad, their number ``n`` and
        ``n_bad``: one sync per epoch where the reference has one per step (train_cf.py:205-210)."""
        s = self.sums.cpu().tolist()
        n = max(s[S_N], 1.0)
        out = dict(loss=s[S_LOSS] / n, aux_loss=s[S_AUX] / n, elbo=s[S_ELBO] / n, nll=s[S_NLL] / n, kl=s[S_KL] / n, n=int(s[S_N]),
                   n_bad=int(s[S_BAD]))
        if reset:
            self.sums.zero_()
        return out

    # -- checkpoint (train_cf.py:516-526) ---------------------------------------------------------------------
    def _model_state(self, vae, lmbda):
        sd = {"vae." + k: v.detach().clone() for k, v in vae.state_dict().items()}
        sd["lmbda"] = lmbda.detach().clone()
        sd["eps"] = self.dscm.eps.detach().clone()
        return sd

    def state_dict(self):
        """``model_state_dict`` / ``ema_model_state_dict`` (the trained part of ``DSCM.state_dict()``: ``vae.*``, ``lmbda``, ``eps``;
        the frozen pgm and predictor keep their own checkpoints), ``optimizer_state_dict`` (flat AdamW moments in the engine's
        parameter order and the device step state) and ``lagrange_opt_state_dict`` (the multiplier's moments)."""
        names = self._names()
        sd = {"step": self.it, "model_state_dict": self._model_state(self.vae, self.lag[LMBDA:LMBDA + 1]),
              "optimizer_state_dict": self.tail.flat_optimizer_state(names),
              "lagrange_opt_state_dict": {"exp_avg": self.lag[LM:LM + 1].clone(), "exp_avg_sq": self.lag[LV:LV + 1].clone(),
                                          "lr": self.lr_lagrange, "maximize": True},
              "cgen": {"sums": self.sums.clone(), "rng": self.eng.rng.clone() if getattr(self.eng, "rng", None) is not None else None}}
        if self.ema_model is not None:
            sd["ema_model_state_dict"] = self._model_state(self.ema_vae, self.lag[LEMA:LEMA + 1])
        return sd

    def _names(self):
        by_id = {id(p): n for n, p in self.vae.named_parameters()}
        return [by_id[id(p)] for p in self.eng.params]

    def _load_model(self, vae, slot, sd):
        vae.load_state_dict({k[4:]: v for k, v in sd.items() if k.startswith("vae.")}, strict=True)  # (in place: the flat views stay)
        self.lag[slot:slot + 1].copy_(sd["lmbda"].reshape(1))

    def load_state_dict(self, sd):
        self._load_model(self.vae, LMBDA, sd["model_state_dict"])
        if self.ema_model is not None and "ema_model_state_dict" in sd:
            self._load_model(self.ema_vae, LEMA, sd["ema_model_state_dict"])
        self.tail.load_flat_optimizer_state(sd["optimizer_state_dict"], self._names())
        self.lag[LM:LM + 1].copy_(sd["lagrange_opt_state_dict"]["exp_avg"].reshape(1))
        self.lag[LV:LV + 1].copy_(sd["lagrange_opt_state_dict"]["exp_avg_sq"].reshape(1))
        extra = sd.get("cgen") or {}
        if extra.get("sums") is not None:
            self.sums.copy_(extra["sums"])
        if extra.get("rng") is not None:
            self.eng.rng_ptr()
            self.eng.rng.copy_(extra["rng"])
        self.it = int(sd.get("step", 0))
        self._mark_weights_written()
