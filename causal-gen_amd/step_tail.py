"""What the device-side training steps (``train.TrainStep``, ``predictor_train.PredictorTrainStep``, ``pgm_train.PgmTrainStep``)
have in common: the optimiser tail of csrc/optim.hip as one launch sequence (``StepTail``), the names of its state vector, the
eager-first-then-capture helper, and the flattening of a module's parameters into one f32 buffer.  A step owns its forward and
backward pass, its graph keys and its data-parallel exchange; everything after the gradient is here.
"""
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
