"""What the device-side training steps (``train.TrainStep``, ``cf_train.CfTrainStep``, ``predictor_train.PredictorTrainStep``,
``predictor_resnet_train.ChestPredictorTrainStep``, ``pgm_train.PgmTrainStep``) have in common: the optimiser tail of csrc/optim.hip
as one launch sequence (``StepTail``), the names of its state vector, the eager-first-then-capture helper, and the flattening of a
module's parameters into one f32 buffer.  A step owns its forward and backward pass, its graph keys and its data-parallel exchange;
everything after the gradient is here.

The three supervised steps (stages one and two of the pipeline) share more than the tail, and that is here too: ``SupStep`` is
their skeleton -- hyper-parameters, EMA copy, the two ``Flat``s, gradient buffer and tail, ``_optim``, the eager-first-then-replay
``_run``, the gradient dictionary and the checkpoint pair; a subclass brings ``_flatten``, ``_fwd_bwd`` and its static entries.
``ImageSupStep`` adds what the two image steps share: the staging of observation columns for ``step`` and the data-set half of
``step_from``.  ``TrainStep`` and ``CfTrainStep`` are driven by the engine, key their graphs differently and return other things:
they use the tail and the helpers, not the skeleton.
"""
import copy
import ctypes as C
from collections import namedtuple

import torch

from . import _lib

# hipGraph captures are THREAD-LOCAL: with a ProcessGroupNCCL alive, its watchdog thread polls events (hipEventQuery) at any
# moment, which a capture in the default "global" mode treats as an illegal call and dies of ("operation failed due to a previous
# error during capture") -- found by tools/dp_rccl_dryrun.py, invisible to the gloo tests
CAPTURE_MODE = "thread_local"

# The step state: 8 floats on the device.  csrc/optim.hip owns this layout (clip_decide writes 0-4 and 6, step_commit 5, adamw_ema
# reads 2, 3 and 5); the last float is not the kernels'.
SUMSQ, NORM, CLIP_COEF, SKIP, N_SKIPPED, OPT_STEPS, N_NONFINITE = range(7)
STATE_FLOATS = 8


def check_warmup(n):
    """Before any device work: the kernel's LambdaLR(linear_warmup) divides by the warm-up length."""
    if int(n) <= 0:
        raise ValueError(f"lr_warmup_steps must be > 0 (got {n}): the linear warm-up divides by it")


def normalize_columns(columns):
    """``columns=`` of a step's ``step_from``: {variable: column of ds.pa, or (first column, width)} as {variable: (first column,
    width)} (cf_eval.predictor_eval's convention); None stays None."""
    return None if columns is None else {k: (int(v), 1) if isinstance(v, int) else (int(v[0]), int(v[1])) for k, v in columns.items()}


def check_index(index, who):
    if index.dtype != torch.int64 or index.dim() != 1 or index.device.type != "cuda":
        raise ValueError(f"{who}: the index must be a device int64 vector")


def flatten(tensors, dev):
    """One f32 buffer holding `tensors` back to back; each tensor's ``.data`` becomes a view of it.  Returns (flat, offsets)."""
    flat = torch.empty(sum(t.numel() for t in tensors), dtype=torch.float32, device=dev)
    offs, o = [], 0
    for t in tensors:
        k = t.numel()
        flat[o:o + k].copy_(t.detach().reshape(-1).float())
        t.data = flat[o:o + k].view(t.shape)
        offs.append(o)
        o += k
    return flat, offs


class Flat:
    """Named parameters flattened into one f32 buffer: ``names``, ``params``, ``flat_p``, ``p_off`` (online model or EMA copy)."""

    def __init__(self, named, dev):
        named = list(named)
        self.names, self.params = [n for n, _ in named], [p for _, p in named]
        self.flat_p, self.p_off = flatten(self.params, dev)

    def invalidate(self):
        """After the kernels have written the parameters through raw pointers: drop what the owner cached of their old values."""


def ranges_where(eng, pred):
    """Contiguous [lo, hi) ranges of an engine's flat buffers covered by the parameters `pred` holds for (neighbours are joined)."""
    rs, cur = [], None
    for p in eng.params:
        o, k = eng.p_off[id(p)], p.numel()
        if not pred(p):
            cur = None
        elif cur is not None and cur[1] == o:
            cur[1] = o + k
        else:
            cur = [o, o + k]
            rs.append(cur)
    return [(a, b) for a, b in rs]


def mark_weights_written(*models):
    """The fused AdamW / EMA kernel writes the flat parameter buffers through raw pointers, which torch's version counters do not
    see: tell the engines of `models` (None entries allowed) that their weight images are stale, so the next inference call
    re-images before it runs."""
    for mod in models:
        eng = None if mod is None else mod.__dict__.get("_eng")
        if eng is not None:
            eng.weights_dirty = True


def pin_drop_cond(model):
    """``drop_cond`` of a conditional-prior decoder is a host draw: draw it, pin the outcome for this step's launches and return
    it (a captured step is keyed by it)."""
    drop = type(model.decoder).drop_cond(model.decoder)
    model.decoder.__dict__["drop_cond"] = lambda d=drop: d
    return drop


def capture(fn):
    """`fn()` captured into a hipGraph, after an eager run of the same launches by the caller.  Returns (graph, fn's result)."""
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode=CAPTURE_MODE):
        out = fn()
    return g, out


# AdamW(lr, betas, eps, wd) under LambdaLR(linear_warmup(lr_warmup_steps)), clip_grad_norm_(grad_clip) and an EMA(ema_rate) with
# update_after_step = ema_update_after; a norm at or above grad_skip drops the step (inf: only a non-finite one or a NaN loss does)
# `const_lr` (defaulted: the nine-field constructions mean what they always did): no LambdaLR, `lr` on every step, `lr_warmup_steps`
# unused -- train_cf.py has no scheduler, and linear_warmup(n) would give the first step lr = 0 for every n >= 1
HyperParams = namedtuple("HyperParams", "lr betas eps wd grad_clip grad_skip lr_warmup_steps ema_rate ema_update_after const_lr",
                         defaults=(False,))


class StepTail:
    """Global grad-norm -> clip / skip predicate -> fused AdamW + EMA -> step counter commit, on flat f32 buffers of `n` elements.
    Owns the moments ``m`` / ``v``, the step ``state`` and the norm's ``partial`` sums (`norm_blocks` of them: their number fixes
    the order of the norm's sum, hence its bits).  `extra_norm_slots`: further sums of squares that belong to the norm and lie outside
    the flat gradient (``extra_slot(i)`` is where their owner writes them before ``run``; ``cgen_sumsq_partial`` fills the first
    `norm_blocks` entries, ``cgen_clip_decide`` sums all)."""

    def __init__(self, lib, n, device, norm_blocks, extra_norm_slots=0):
        self.lib, self.n, self.norm_blocks, self.extra_norm_slots = lib, n, norm_blocks, int(extra_norm_slots)
        self.m = torch.zeros(n, device=device)
        self.v = torch.zeros(n, device=device)
        self.state = torch.zeros(STATE_FLOATS, device=device)
        self.partial = torch.zeros(norm_blocks + self.extra_norm_slots, device=device)
        self._zero = None  # zero gradient / moments of the `ema_only` passes

    def _adamw(self, hp, p, g, m, v, ema, count, lr, wd, stream):
        q = _lib.AdamwArgs()
        q.p, q.g, q.m, q.v, q.ema, q.count = p, g, m, v, ema, count
        q.lr, q.beta1, q.beta2, q.eps, q.wd = lr, hp.betas[0], hp.betas[1], hp.eps, wd
        q.ema_beta, q.warmup_steps, q.ema_update_after = hp.ema_rate, hp.lr_warmup_steps, hp.ema_update_after
        q.state_dev = self.state.data_ptr()
        (self.lib.adamw_ema_const_lr if hp.const_lr else self.lib.adamw_ema)(C.byref(q), stream)

    def extra_slot(self, i):
        """Device address of the i-th extra sum-of-squares slot of the norm."""
        if not 0 <= i < self.extra_norm_slots:
            raise IndexError(f"StepTail: extra norm slot {i} of {self.extra_norm_slots}")
        return self.partial.data_ptr() + 4 * (self.norm_blocks + i)

    def run(self, hp, p, g, ema, out3, stream, ranges=None, ema_only=(), before_commit=None):
        """One optimiser step of the flat parameters `p` on the flat gradient `g` (`ema`: the averaged copy, or None).  `out3`
        (or None): device [elbo, nll, kl], a NaN in nll or kl drops the step.  `ranges`: the [lo, hi) element ranges to update,
        one launch each (default: everything); the norm is always of the whole of `g`.  `ema_only`: (p_ptr, ema_ptr, count)
        regions that are averaged with the step's decay and otherwise left alone (lr = wd = 0 on a zero gradient).
        `before_commit(stream)`: launches of the caller's between the last ``adamw_ema`` and ``step_commit`` -- they see this step's
        clip coefficient and skip flag and the count of successful steps BEFORE it, as ``adamw_ema`` does."""
        lib, state = self.lib, self.state.data_ptr()
        lib.sumsq_partial(g.data_ptr(), g.numel(), self.partial.data_ptr(), self.norm_blocks, stream)
        lib.clip_decide(self.partial.data_ptr(), self.norm_blocks + self.extra_norm_slots, None if out3 is None else out3.data_ptr(), hp.grad_clip,
                        hp.grad_skip, state, stream)
        for lo, hi in [(0, g.numel())] if ranges is None else ranges:
            self._adamw(hp, p.data_ptr() + 4 * lo, g.data_ptr() + 4 * lo, self.m.data_ptr() + 4 * lo, self.v.data_ptr() + 4 * lo,
                        None if ema is None else ema.data_ptr() + 4 * lo, hi - lo, hp.lr, hp.wd, stream)
        for p_ptr, ema_ptr, count in ema_only:
            if self._zero is None:  # (in the eager first step: captured graphs hold its address, so it never moves)
                self._zero = torch.zeros(3, max(count, 1), device=self.state.device)
            z = self._zero
            if z.shape[1] < count:
                raise ValueError(f"StepTail: an ema_only region of {count} elements after one of {z.shape[1]}")
            self._adamw(hp, p_ptr, z[0].data_ptr(), z[1].data_ptr(), z[2].data_ptr(), ema_ptr, count, 0.0, 0.0, stream)
        if before_commit is not None:
            before_commit(stream)
        lib.step_commit(state, stream)

    def stats(self):
        """Host read of the device-side step state (one sync; call every N steps, not every step)."""
        return self.stats_of(self.state.cpu().tolist())

    @staticmethod
    def stats_of(s):
        """``stats()`` from the state vector's floats already on the host (a caller that reads more in the same copy)."""
        return dict(grad_norm=s[NORM], clip_coef=s[CLIP_COEF], skipped_last=bool(s[SKIP]), n_skipped=int(s[N_SKIPPED]),
                    opt_steps=int(s[OPT_STEPS]))

    def flat_optimizer_state(self, names):
        """The flat AdamW moments (in the order of `names`) and the device step state, for a checkpoint."""
        return {"exp_avg": self.m.clone(), "exp_avg_sq": self.v.clone(), "state": self.state.clone(), "names": list(names)}

    def load_flat_optimizer_state(self, sd, names):
        if list(sd.get("names", names)) != list(names):
            raise ValueError("load_state_dict: the optimiser state belongs to other parameters")
        self.m.copy_(sd["exp_avg"])
        self.v.copy_(sd["exp_avg_sq"])
        self.state.copy_(sd["state"])


class SupStep:
    """The skeleton of a supervised training step: one model, its EMA copy, one flat gradient and the tail, run eagerly once per
    static entry and replayed from a hipGraph afterwards.  A subclass gives ``NORM_BLOCKS``, ``_flatten(model, dev)`` (the ``Flat``
    of a model; called for the EMA copy first, the online model second) and ``_fwd_bwd(ent)`` (every launch up to the gradient
    of loss / B in ``flat_g``, the summed loss in ``out3[1]`` and the mean loss in ``res[0]``), and may override ``_ema_only``
    and the four checkpoint hooks below ``state_dict``."""

    def __init__(self, model, lr, wd, betas, eps, grad_clip, lr_warmup_steps, ema_rate, ema, use_graph, ema_update_after, device):
        check_warmup(lr_warmup_steps)
        self.lib = _lib.require_gpu()
        dev = self.device = torch.device(device)
        # (no norm threshold in sup_epoch: only a non-finite norm or a NaN loss drops the step)
        self.hp = HyperParams(float(lr), (float(betas[0]), float(betas[1])), float(eps), float(wd), float(grad_clip), float("inf"),
                              int(lr_warmup_steps), float(ema_rate), int(ema_update_after))
        self.use_graph = use_graph
        self.ema_model = self._ema = None
        if ema:
            self.ema_model = copy.deepcopy(model)
            self.ema_model.requires_grad_(False)
            self._ema = self._flatten(self.ema_model, dev)
        self.model = model
        self._on = self._flatten(model, dev)
        n = self._on.flat_p.numel()
        self.flat_g = torch.zeros(n, device=dev)
        self.tail = StepTail(self.lib, n, dev, self.NORM_BLOCKS)
        self.stats = self.tail.stats  # host read of the device-side step state (one sync)
        self.m, self.v, self.state, self.partial = self.tail.m, self.tail.v, self.tail.state, self.tail.partial
        self.out3 = torch.zeros(3, device=dev)  # [-, summed loss (PgmTrainStep: log-probability), 0]: what cgen_clip_decide tests for NaN
        self.res = torch.zeros(2, device=dev)   # [mean loss, gradient norm] of the last step
        self._statics, self._graphs = {}, {}
        self.it = 0

    # -- pieces -------------------------------------------------------------------------------------------
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _ema_only(self):
        """(p_ptr, ema_ptr, count) regions that are averaged into the EMA copy and otherwise left alone (``StepTail.run``)"""
        return ()

    def _optim(self):
        self.tail.run(self.hp, self._on.flat_p, self.flat_g, None if self._ema is None else self._ema.flat_p, self.out3, self._stream(),
                      ema_only=self._ema_only())
        self.res[1:2].copy_(self.state[NORM:NORM + 1])

    def _fwd_bwd_optim(self, ent):
        self._fwd_bwd(ent)
        self._optim()

    def _invalidate(self):
        self._on.invalidate()
        if self._ema is not None:
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

    def _grads(self):
        """{parameter name: a copy of its part of the flat gradient}"""
        on = self._on
        return {n: self.flat_g[o:o + p.numel()].view(p.shape).clone() for n, p, o in zip(on.names, on.params, on.p_off)}

    # -- checkpoint ---------------------------------------------------------------------------------------
    def state_dict(self):
        """The reference checkpoint's keys (train_pgm.py:536-545): ``model_state_dict`` / ``ema_model_state_dict`` with the
        reference's parameter names, ``optimizer_state_dict`` (flat AdamW moments in the order of ``_on.names`` and the device
        step state), and what ``_extra_state`` adds."""
        sd = {"step": self.it, "model_state_dict": {k: v.detach().clone() for k, v in self.model.state_dict().items()},
              "optimizer_state_dict": self.tail.flat_optimizer_state(self._on.names), **self._extra_state()}
        if self.ema_model is not None:
            sd["ema_model_state_dict"] = {k: v.detach().clone() for k, v in self.ema_model.state_dict().items()}
        return sd

    def load_state_dict(self, sd):
        self._load_model(self.model, sd["model_state_dict"])  # (copies in place: the flat views stay)
        if self.ema_model is not None and "ema_model_state_dict" in sd:
            self._load_model(self.ema_model, sd["ema_model_state_dict"])
        opt = self._optimizer_state(sd)
        if opt is not None:
            self.tail.load_flat_optimizer_state(opt, self._on.names)
        self._load_extra_state(sd)
        self.it = int(sd.get("step", 0))
        self._invalidate()

    def _extra_state(self):
        return {}

    def _load_extra_state(self, sd):
        pass

    def _load_model(self, model, sd):
        model.load_state_dict(sd, strict=True)

    def _optimizer_state(self, sd):
        """The optimiser state to load, or None to leave the moments (here: a checkpoint without one is an error)"""
        return sd["optimizer_state_dict"]


class ImageSupStep(SupStep):
    """What the two anticausal-predictor steps share on top: ``columns=``, the staging of a batch given by variable (``step``) and
    the data-set half of ``step_from``.  A subclass gives ``_variables()`` (every variable it reads), ``_check_batch(B)``,
    ``_build(x, at, dense)`` (the static entry of a batch shape reading the static image `x`; it holds ``x``) and may refuse a
    data set's geometry in ``_check_geometry``."""

    def __init__(self, model, columns, **kw):
        # {variable: (first column of ds.pa, width)} for step_from
        self.columns = normalize_columns(columns)
        super().__init__(model, **kw)

    def _new_rng(self):
        """A Philox state {seed, offset} of the step's own, seeded from ``torch.initial_seed()``"""
        return torch.tensor([torch.initial_seed() & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64, device=self.device)

    def _cols(self, obs, B):
        """{variable: [B, k] f32} of every observed / context variable the step reads"""
        out = {}
        for var in self._variables():
            if var not in obs:
                raise KeyError(f"{type(self).__name__}: observation {var!r} is missing")
            out[var] = obs[var].detach().reshape(B, -1).float()
        return out

    def _check_geometry(self, ds, r_h, r_w):
        pass

    def _stage(self, x, obs):
        """(key, entry) of a batch shape for ``step``: static input buffers and what ``_build`` makes of them; the prepared image
        `x` and the columns of `obs` are copied into the buffers."""
        name, cols = type(self).__name__, self._cols(obs, int(x.shape[0]))
        key = tuple(x.shape)
        ent = self._statics.get(key)
        if ent is None:
            sc = {k: torch.empty(v.shape, device=self.device) for k, v in cols.items()}
            at = lambda var: (sc[var].data_ptr(), sc[var].shape[1], sc[var].shape[1])  # noqa: E731
            ent = self._statics[key] = self._build(torch.empty_like(x, device=self.device), at, sc)
            ent["cols"] = sc
        ent["x"].copy_(x, non_blocking=True)  # (device to device: _prep_x has moved the image)
        for k, v in cols.items():
            if v.shape != ent["cols"][k].shape:
                raise ValueError(f"{name}: observation {k!r} changed shape from {tuple(ent['cols'][k].shape)} to {tuple(v.shape)}")
            # a host column may be a temporary of _cols: only a copy that has finished may let go of it
            ent["cols"][k].copy_(v, non_blocking=v.is_cuda)
        return key, ent

    def _static_from(self, ds, index, train, draws_out):
        """(key, entry) of a (data set, batch size): static image, gathered parents rows ``pa`` and index, and the augment launch's
        arguments ``aug``.  ``_build``'s ``at(var)`` points into the parents rows (no `dense` buffers: a subclass that needs a
        contiguous copy of a variable makes it inside the step)."""
        who = f"{type(self).__name__}.step_from"
        if self.columns is None:
            raise ValueError(f"{who}: name the columns of ds.pa at construction (columns={{variable: column}})")
        missing = [v for v in self._variables() if v not in self.columns]
        if missing:
            raise ValueError(f"{who}: no column was named for {missing}")
        check_index(index, who)
        B = int(index.numel())
        self._check_batch(B)
        if draws_out is not None:
            assert draws_out.dtype == torch.int32 and tuple(draws_out.shape) == (B, 3) and draws_out.is_contiguous() and draws_out.is_cuda
        key = (ds.key(train), B, None if draws_out is None else draws_out.data_ptr())
        ent = self._statics.get(key)
        if ent is None:
            dev = self.device
            for var in self._variables():
                c0, k = self.columns[var]
                if not 0 <= c0 <= ds.ctx - k:
                    raise ValueError(f"{who}: variable {var!r}: columns {c0}..{c0 + k - 1} do not fit ds.pa's {ds.ctx}")
            r_h, r_w, _, _, _ = ds.geometry(train)
            self._check_geometry(ds, r_h, r_w)
            x = torch.empty((B, ds.c, r_h, r_w), device=dev)
            pa = torch.zeros((B, ds.ctx), device=dev)
            ent = self._statics[key] = self._build(x, lambda var: (pa.data_ptr() + 4 * self.columns[var][0], ds.ctx, self.columns[var][1]), None)
            if self._rng is None:
                self._rng = self._new_rng()
            # one channel: NHWC and planar are the same memory and the existing launch serves; else the planar one
            view = _lib.View(x.data_ptr(), r_h * r_w, r_w, 1, 1, 0) if ds.c == 1 else ds.planar_view(x.data_ptr(), train)
            index_buf = torch.zeros(B, dtype=torch.int64, device=dev)
            args = ds.args_for(_lib.F32, B, index_buf.data_ptr(), view, self._rng.data_ptr(), train, None,
                               None if draws_out is None else draws_out.data_ptr(), pa.data_ptr())
            ent.update(pa=pa, index=index_buf, aug=args, train=train, keep=(ds, draws_out))
        ent["index"].copy_(index, non_blocking=True)
        return key, ent
