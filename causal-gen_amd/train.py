"""The per-step training harness of the reference (trainer.py:49-87, train_setup.py:42-53, utils.py:87-228) as a
fixed launch sequence on the GPU:

    weight images -> HVAE forward -> hand-written backward -> [DP: gradient all-reduce] -> global grad-norm ->
    clip / NaN-or-norm skip predicate (on device) -> fused AdamW + EMA -> step counter commit

No autograd, no host synchronisation inside the step (the reference has three): the skip decision,
the LR warm-up, Adam's bias correction and the EMA warm-up schedule are all evaluated on the device from a
device-side count of successful steps.  The whole sequence is captured in a hipGraph after one eager step.
Under data parallelism (one process per GPU, RCCL over xGMI) the flat f32 gradient is averaged across ranks in
buckets between the backward and the norm; ranks share the seed-driven draws and the skip flag by construction
(the flag is a function of the all-reduced gradient and of the all-reduced nll/kl).
"""
import contextlib
import copy
import math
import os
from collections import namedtuple

import torch

from . import _lib, dp
from .engine import StaticParents, compact_parents
from .step_tail import (CAPTURE_MODE, N_NONFINITE, N_SKIPPED, OPT_STEPS, STATE_FLOATS, HyperParams, StepTail, capture, check_warmup,
                        mark_weights_written, pin_drop_cond, ranges_where)


def preprocess_batch(args, batch, expand_pa=False):
    """trainer.py:16-21 on the device: u8 pixels -> [-1, 1] f32 (one HIP launch, no ATen arithmetic), parents to f32 and,
    for the HVAE's parent concatenation, broadcast to [B, ctx, R, R] -- as a stride-0 ``expand`` view, not a ``repeat``: same
    shape and values for every consumer, and the HVAE then lays out only the [B,1,1,ctx] vector (engine.from_parents).
    ``HVAE.forward`` also accepts the raw u8 batch directly and fuses the normalisation into its NCHW -> NHWC load, which
    skips this pass altogether."""
    lib = _lib.require_gpu()
    dev = torch.device(getattr(args, "device", "cuda"))
    x = batch["x"].to(dev)
    if x.dtype == torch.uint8:
        x = x.contiguous()
        n, c, h, w = x.shape
        out = torch.empty((n, h, w, c), dtype=torch.float32, device=dev)  # channels-last memory, NCHW shape below
        lib.nchw_to_nhwc(1, _lib.F32, n, c, h, w, x.data_ptr(), _lib.View(out.data_ptr(), h * w * c, w * c, c, c, 0), 127.5,
                         1.0 / 127.5, torch.cuda.current_stream(dev).cuda_stream)
        x = out.permute(0, 3, 1, 2)
    else:
        x = (x.float() - 127.5) / 127.5
    batch["x"] = x
    batch["pa"] = batch["pa"].to(dev).float()
    if expand_pa:
        batch["pa"] = batch["pa"][..., None, None].expand(-1, -1, *(args.input_res,) * 2)
    return batch


def _covers(have, want):
    """True when every [lo, hi) of `want` lies inside one range of `have` (both sorted, disjoint)."""
    return all(any(a <= lo and hi <= b for a, b in have) for lo, hi in want)


def _subtract_ranges(whole, holes):
    """[lo, hi) ranges of `whole` not covered by `holes` (both sorted, non-overlapping)."""
    out = []
    for lo, hi in whole:
        cur = lo
        for a, b in holes:
            if b <= cur or a >= hi:
                continue
            if a > cur:
                out.append((cur, a))
            cur = max(cur, b)
        if cur < hi:
            out.append((cur, hi))
    return out


def linear_warmup(warmup_iters):
    """utils.py:32-36."""
    return lambda it: 1.0 if it > warmup_iters else it / warmup_iters


# A captured step: ``g1`` forward + backward (on one GPU also the optimiser tail, under data parallelism ``g2``; ``g1b``: the
# backward pass after the overlapped form's cut), the static batch and parents (None: a device-side input) and [elbo, nll, kl]
GraphEntry = namedtuple("GraphEntry", "g1 g2 sx spb so g1b")


class TrainStep:
    NORM_BLOCKS = 1024

    def __init__(self, model, args, ema=True, use_graph=True, process_group=None, bucket_mb=32):
        check_warmup(args.lr_warmup_steps)
        self.model, self.args = model, args
        self.lib = _lib.require_gpu()  # (the step tail's own kernels; the model's launches go through eng.lib, the staging proxy)
        self.use_graph = use_graph
        self.pg = process_group
        self.world = torch.distributed.get_world_size(process_group) if process_group is not None else 1
        self.bucket_elems = int(bucket_mb * (1 << 20) // 4)
        # the data-parallel machinery (communication stream, split backward graph, bucketed all-reduce) is active with more than
        # one rank -- or, for a dry run of exactly that code through RCCL on ONE GPU, with CGEN_DP_FORCE=1 and a 1-rank group
        self.dp = self.world > 1 or (process_group is not None and os.environ.get("CGEN_DP_FORCE") == "1")
        if self.dp and getattr(model, "free_bits", 0) > 0:
            self.use_graph = False  # free bits exchange per-channel KL sums inside the forward pass (vae.py): not capturable
        model.train()
        eng = model.engine()
        self.eng = eng
        n = eng.flat_p.numel()
        dev = eng.device
        self.tail = StepTail(self.lib, n, dev, self.NORM_BLOCKS)
        self.m, self.v, self.state, self.partial = self.tail.m, self.tail.v, self.tail.state, self.tail.partial
        self.ema_model = None
        if ema:
            self.ema_model = copy.deepcopy(model).to(dev)
            self.ema_model.requires_grad_(False)
            self.ema_model.eval()
            self.ema_flat = self.ema_model.engine().flat_p
        self.coefs = {}   # (B, dims) -> [device tensor (1/(B dims accu), beta/(B dims accu), beta), beta last written]
        self.coef = None
        self.ranges = None
        self.graphs = {}
        self.inputs = {}  # step_from: (data set, batch size, train, draws tap) -> data.AugmentedInput (static index / parents buffers)
        self.beta = float(args.beta)
        self.it = 0
        # DP: the gradient exchange either follows the backward graph (serialized: graph | bucketed all-reduce | optimiser graph)
        # or travels under it (overlap: the backward graph is cut where the decoder half of the gradient is final, that half is
        # exchanged on the communication stream under the encoder's backward pass).  Overlap is not free: it needs a second
        # background weight-gradient flush (+0.35 ms) and a third graph, +1.0 ms per step on ukbb192 measured on one MI355X
        # through a 1-rank RCCL group (tools/dp_rccl_dryrun.py, bench.py with CGEN_DP_FORCE=1: 18.43 vs 17.39 ms), while the
        # serialized exchange of its 69.5 MB costs ~0.4 ms on an xGMI node (2 (N-1)/N x bytes at ~300 GB/s bus bandwidth).
        # CGEN_DP_OVERLAP=1 / 0 forces a form; unset, the step overlaps only when the estimated exchange exceeds that price.
        _ov = os.environ.get("CGEN_DP_OVERLAP")
        if _ov is None:
            est_s = 4.0 * n * 2.0 * max(self.world - 1, 0) / max(self.world, 1) / float(os.environ.get("CGEN_DP_BUS_GBS", "300")) / 1e9
            self.dp_overlap = self.dp and est_s > 1.0e-3
            self.dp_policy = "auto: estimated exchange %.2f ms %s the ~1 ms the overlapped form costs" % (1e3 * est_s, ">" if self.dp_overlap else "<=")
        else:
            self.dp_overlap = self.dp and _ov != "0"
            self.dp_policy = "forced by CGEN_DP_OVERLAP=" + _ov
        if self.dp_overlap:
            # a second background flush at the end of the DECODER's backward pass (75.5 % of the weight-gradient work of the
            # 192^2 presets; costs 0.8 % on one GPU): from there on every decoder / likelihood gradient is final -- 48 of the
            # 69.5 MB of ukbb192 -- and is exchanged under the encoder's backward pass; the graph is cut at 90 %
            if "CGEN_WGRAD_FLUSH_FRAC" not in os.environ:
                eng.wgrad_flush_frac = [0.55, 0.755]
            if "CGEN_DP_SPLIT_FRAC" not in os.environ:
                eng.split_frac = 0.9
        self.comm_stream = None
        self.early_ranges = self.late_ranges = None
        self._early_ok = True
        self.time_comm = False
        self._comm_events = []
        # gradient accumulation (trainer.py:64-67): elbo / accu_steps per iteration, summed in a second flat buffer; the
        # optimiser tail runs on iterations with (it - 1) % accu_steps == 0 and reads that buffer
        self.accu = max(1, int(getattr(args, "accu_steps", 1) or 1))
        # f16 loss-scale back-off: looked after INSIDE step(), on every rank, every `ls_check_interval` iterations,
        # keyed by the iteration counter (idempotent); stats() is read-only.  The decision reads the device state of the
        # previous step, which is identical on all data-parallel ranks (all-reduced gradient + scalars feed clip_decide).
        self.overflow_backoffs, self._clean_checks, self.ls_growth_interval = 0, 0, 20
        self.ls_check_interval, self._ls_checked_it, self._ls_last_growth_it = 16, 0, None
        self._ls_nonfinite_seen = 0.0  # state[N_NONFINITE] (steps dropped for a non-finite norm) at the previous check
        self.LS_SHIFT_MIN = -16
        self.acc_g = torch.zeros(n, device=dev) if self.accu > 1 else None

    # -- pieces -----------------------------------------------------------------------------------------
    def _coef_for(self, x, beta):
        """Per-(batch, dims) device constants of a step: gradient seeds d(elbo)/d(sum nll), d(elbo)/d(sum kl) and beta itself.
        They live in device memory so that a captured step follows the beta warm-up (trainer.py:57) without re-capture:
        the host rewrites the three floats (outside any capture) only when beta moved.  One tensor per key, kept alive as
        long as the TrainStep: captured graphs hold its address."""
        B, dims = int(x.shape[0]), float(math.prod(x.shape[1:]))
        ent = self.coefs.get((B, dims))
        if ent is None:
            ent = self.coefs[(B, dims)] = [torch.zeros(3, device=self.eng.device), None]
        if ent[1] != beta:
            S = self.eng.set_loss_scale(B * dims * self.accu)  # (1 for f32; divided out again by the parameter-gradient reduces)
            ent[0].copy_(torch.tensor([S / (B * dims * self.accu), S * beta / (B * dims * self.accu), beta], dtype=torch.float32))
            ent[1] = beta
        return ent[0]

    def _fwd_bwd(self, x, pa, beta, on_split=None):
        m, eng = self.model, self.eng
        dims = float(math.prod(x.shape[1:]))
        self.coef = self.coefs[(int(x.shape[0]), dims)][0]  # written by step() before any capture / replay
        eng.set_loss_scale(int(x.shape[0]) * dims * self.accu)
        m.__dict__["_beta_dev"] = self.coef.data_ptr() + 8
        try:
            out3 = m._run_forward(x, pa, beta, record=True)
        finally:
            m.__dict__["_beta_dev"] = None
        params, xin, B, R, Cx, dims = m.__dict__["_saved"]
        eng.kl_coef_ptr = self.coef.data_ptr() + 4
        eng.like_coef_ptr = self.coef.data_ptr()
        fused = m.__dict__.get("_like_fused", False)
        gparams = None if fused else eng.seed_grad(params)
        if fused:  # the head's tape entry runs the NLL's backward itself, with like_coef_ptr (engine._bw_like_head)
            pass
        elif getattr(m.likelihood, "logit_space", False):
            u, snap = m.__dict__["_gauss_noise"][:2]
            self.lib.gauss_nll_bwd(eng.dt, B, R, R, Cx, params.cv(), xin.cv(), u, snap.data_ptr(), 977, self.coef.data_ptr(), 0,
                                   gparams.cv(), eng.stream)
        elif m.likelihood.kind == "dgauss":
            self.lib.dgauss_nll_bwd(eng.dt, B, R, R, Cx, params.cv(), xin.cv(), self.coef.data_ptr(), 0, gparams.cv(), eng.stream)
        else:
            self.lib.dmol_nll_bwd(eng.dt, B, R, R, params.cv(), xin.cv(), self.coef.data_ptr(), 0, gparams.cv(), eng.stream)
        eng.on_split = on_split  # (called from inside the backward pass, where the early half of the gradient is final)
        try:
            eng.backward()
        finally:
            eng.on_split = None
        if self.acc_g is not None:
            eng.flat_axpy(eng.flat_g.data_ptr(), self.acc_g.data_ptr(), eng.flat_g.numel())
        return out3

    def _gbuf(self):
        return self.eng.flat_g if self.acc_g is None else self.acc_g

    def _allreduce(self, out3):
        """Average the flat gradient (and the reported scalars, whose NaN-ness feeds the skip predicate) over the
        data-parallel ranks: a few large buckets, not 800 small tensors (xGMI rings are per-link bound)."""
        if self.dp:
            with self._comm_timed():  # (serialized form: the whole exchange is exposed)
                dp.bucketed_allreduce_mean(self._gbuf(), self.bucket_elems, self.pg, extra=(out3,))

    @contextlib.contextmanager
    def _comm_timed(self):
        """With ``time_comm``: an event pair around the part of the gradient exchange the step waits for (``exposed_comm_ms``)."""
        timed = self.time_comm
        if timed:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
        yield
        if timed:
            t1.record()
            self._comm_events.append((t0, t1))

    def _ranges_where(self, pred):
        """Contiguous [lo, hi) ranges of the flat buffers covered by the parameters `pred` holds for (neighbours are joined)."""
        return ranges_where(self.eng, pred)

    # -- gradient all-reduce overlapped with the backward pass (north_star) -------------------------
    def _allreduce_ranges(self, ranges, works):
        """Issue the asynchronous all-reduce (a sum) of these ranges of the flat gradient, a bucket at a time, onto `works`."""
        g = self._gbuf()
        for lo, hi in ranges:
            for o in range(lo, hi, self.bucket_elems):
                works.append(torch.distributed.all_reduce(g[o:min(hi, o + self.bucket_elems)], group=self.pg, async_op=True))

    def _early_launch(self):
        """Issue the all-reduce of the gradients that are already final (the decoder half, reduced by the background flush) on
        the communication stream, behind everything the main stream has done so far.  Returns the pending work handles."""
        main = torch.cuda.current_stream(self.eng.device)
        if self.comm_stream is None:
            self.comm_stream = torch.cuda.Stream(self.eng.device)
        self.comm_stream.wait_stream(main)
        works = []
        with torch.cuda.stream(self.comm_stream):
            self._allreduce_ranges(self.early_ranges, works)
        return works

    def _late_finish(self, out3, works):
        """All-reduce what the rest of the backward pass produced (plus the reported scalars), wait for both halves, average."""
        with self._comm_timed():
            self._allreduce_ranges(self.late_ranges, works)
            works.append(torch.distributed.all_reduce(out3, group=self.pg, async_op=True))
            for w in works:
                w.wait()
            self._gbuf().mul_(1.0 / self.world)
            out3.mul_(1.0 / self.world)

    def exposed_comm_ms(self):
        """Mean time per step between the end of the backward pass and the end of the gradient exchange (what the all-reduce
        adds to the step; needs ``time_comm = True`` before the steps of interest)."""
        if not self._comm_events:
            return None
        torch.cuda.synchronize()
        v = [a.elapsed_time(b) for a, b in self._comm_events]
        self._comm_events = []
        return sum(v) / len(v)

    def _optim(self, out3):
        eng, a = self.eng, self.args
        eng.stream = torch.cuda.current_stream(eng.device).cuda_stream  # (inside a capture: the capturing stream)
        # (read from `args` at every eager step: an eager run may move them between steps; a captured step has them baked in)
        hp = HyperParams(float(a.lr), (float(a.betas[0]), float(a.betas[1])), 1e-8, float(a.wd), float(a.grad_clip), float(a.grad_skip),
                         int(a.lr_warmup_steps), float(a.ema_rate), 100)
        if self.ranges is None:  # the parameters the backward pass writes a gradient for: the others keep weights and moments
            self.ranges = self._ranges_where(lambda p: id(p) in eng.pgrad_init and p.requires_grad)
        self.tail.run(hp, eng.flat_p, self._gbuf(), self.ema_flat if self.ema_model is not None else None, out3, eng.stream,
                      ranges=self.ranges)
        if self.acc_g is not None:  # model.zero_grad() of trainer.py:87
            eng.flat_axpy(None, self.acc_g.data_ptr(), self.acc_g.numel(), alpha=0.0, accumulate=False)

    def _eager(self, x, pa, beta, do_step=True):
        self._coef_for(x, beta)
        overlap = self.dp_overlap and do_step and self.acc_g is None
        works, fired = [], []
        if overlap:
            def at_split():
                now = self._ranges_where(lambda p: id(p) in self.eng.early_final)
                if self.early_ranges is None:  # first step: which flat ranges are final here, and which come later
                    self.early_ranges = now
                # the ranges are fixed by the FIRST tape; another tape (other batch shape / drop_cond outcome) may cut at a
                # place where some of those gradients are still being written: such a step exchanges everything after the
                # backward pass instead (and its graph is captured without the cut)
                self._early_ok = _covers(now, self.early_ranges)
                if self._early_ok:
                    works.extend(self._early_launch())
                    fired.append(True)
            self._early_ok = True
        out3 = self._fwd_bwd(x, pa, beta, at_split if overlap else None)
        self.eng.stream = torch.cuda.current_stream(self.eng.device).cuda_stream
        if do_step:
            if overlap and self._early_ok:
                if self.early_ranges is None:
                    self.early_ranges = []  # (the split mark was never reached: tiny model) -> everything is "late"
                elif not fired:
                    works.extend(self._early_launch())  # (a step without the background flush, e.g. the profiled one: exchange that half now)
                if self.late_ranges is None:  # (the rest of the WHOLE buffer, the slots of unused parameters included)
                    self.late_ranges = _subtract_ranges([(0, self._gbuf().numel())], self.early_ranges)
                self._late_finish(out3, works)
            else:
                self._allreduce(out3)
            self._optim(out3)
            self._mark_weights_written()
        return out3

    def _mark_weights_written(self):
        """The fused AdamW / EMA kernel writes both flat parameter buffers through raw pointers, which torch's version
        counters do not see: tell the engines (model and EMA copy) that their weight images are stale, so the next
        inference call (validation on ``ema_model``, sampling, counterfactuals) re-images before it runs."""
        mark_weights_written(self.model, self.ema_model)

    # -- public -------------------------------------------------------------------------------------------
    def step(self, x, pa):
        """One optimiser step on a batch already resident on the GPU.  Returns the device tensor [elbo, nll, kl]."""
        return self._step(x, pa)

    def step_from(self, ds, index, train=True, draws_out=None):
        """One optimiser step on the rows `index` (device int64 vector) of a ``data.DeviceDataset``: the augmented batch is built
        inside the step by one ``cgen_batch_augment`` launch -- the first launch after the step's ``rng_advance``, eager and
        captured alike -- which writes the encoder's input tensor in the compute dtype and a static [B, ctx] parents buffer,
        drawing crops and flips from the engine's Philox state without advancing it (the step consumes exactly the state
        advances of ``step()``).  Replays refill a static index buffer, as ``step()`` refills its static batch.  Gradient
        accumulation, data parallelism and the loss-scale back-off are ``step()``'s.
        `draws_out` (debug tap): a device int32 [B, 3] tensor that receives the (oy, ox, flip) used; part of the graph key."""
        key = (id(ds), int(index.numel()), train, None if draws_out is None else draws_out.data_ptr())
        hook = self.inputs.get(key)
        if hook is None:
            from .data import AugmentedInput

            hook = self.inputs[key] = AugmentedInput(ds, int(index.numel()), train, draws_out)
        hook.load(index)
        return self._step(hook, hook.pa_buf)

    def _step(self, x, pa):
        a = self.args
        self._loss_scale_check()
        self.it += 1
        beta = self.beta
        if getattr(a, "beta_warmup_steps", 0) > 0:
            beta = self.beta * linear_warmup(a.beta_warmup_steps)(self.it)
        do_step = (self.it - 1) % self.accu == 0
        if not self.use_graph:
            return self._eager(x, pa, beta, do_step)
        key = self._graph_key(x, pa, do_step)
        ent = self.graphs.get(key)
        self._coef_for(x, beta)
        if ent is None:
            out = self._eager(x, pa, beta, do_step)  # eager warm-up: sizes the arena, builds the tables
            self.graphs[key] = self._capture(x, pa, beta, do_step)
            return out
        return self._replay(ent, x, pa, do_step)

    def _graph_key(self, x, pa, do_step):
        """What a captured step is valid for.  Draws ``drop_cond`` on the host and pins the outcome for this step's launches."""
        m = self.model
        drop = (1, 1)
        if m.cond_prior:  # host draw (shared across DP ranks through the common seed), one graph per outcome
            drop = pin_drop_cond(m)
        # (beta is device data: the warm-up schedule replays the same graph; virtual and materialised parents are different graphs)
        static = hasattr(x, "emit")  # a device-side input (step_from): its buffers are static already, its identity keys the graph
        return (tuple(x.shape), x.dtype, drop, do_step, tuple(pa.shape), compact_parents(pa) is not None, x.key if static else None)

    def _capture(self, x, pa, beta, do_step):
        """The step just run eagerly, captured on static copies of its inputs.  NCCL inside a captured graph is avoided: under DP
        the step is graphs around eager all-reduces (``_replay``)."""
        if hasattr(x, "emit"):
            sx, spb, sp = x, None, pa
        else:
            sx, spb = x.clone(), StaticParents(pa)
            sp = spb.t

        def fwd_bwd():
            so = self._fwd_bwd(sx, sp, beta)
            if not self.dp and do_step:
                self._optim(so)
            return so

        g1b = g2 = None
        if self.dp_overlap and do_step and self.acc_g is None and bool(self.early_ranges) and self._early_ok:
            g1, g1b, so = self._capture_split(sx, sp, beta)
        else:
            g1, so = capture(fwd_bwd)
        if self.dp and do_step:
            g2, _ = capture(lambda: self._optim(so))
        return GraphEntry(g1, g2, sx, spb, so, g1b)

    def _capture_split(self, sx, sp, beta):
        """Forward + backward captured as TWO graphs, cut where the decoder half of the gradient is final (engine.on_split):
        graph A | all-reduce of that half on the communication stream | graph B (rest of the backward pass) | all-reduce of the
        rest | the optimiser's graph.  Returns (A, B or None when the cut was never reached, static out3)."""
        torch.cuda.synchronize()
        g1, g1b = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        cap = torch.cuda.Stream(self.eng.device)
        cap.wait_stream(torch.cuda.current_stream(self.eng.device))
        fired = []

        def at_split():
            g1.capture_end()
            g1b.capture_begin(pool=g1.pool(), capture_error_mode=CAPTURE_MODE)
            fired.append(True)

        with torch.cuda.stream(cap):
            g1.capture_begin(capture_error_mode=CAPTURE_MODE)
            so = self._fwd_bwd(sx, sp, beta, at_split)
            (g1b if fired else g1).capture_end()
        torch.cuda.current_stream(self.eng.device).wait_stream(cap)
        return g1, g1b if fired else None, so

    def _replay(self, ent, x, pa, do_step):
        if ent.spb is not None and ent.sx.data_ptr() != x.data_ptr():
            ent.sx.copy_(x, non_blocking=True)
            ent.spb.load(pa)
        ent.g1.replay()
        if ent.g1b is not None:
            works = self._early_launch()
            ent.g1b.replay()
            self._late_finish(ent.so, works)
            ent.g2.replay()
        elif ent.g2 is not None:
            self._allreduce(ent.so)
            ent.g2.replay()
        if do_step:
            self._mark_weights_written()
        return ent.so

    # -- checkpoint / resume (trainer.py:154-165, main.py:75-90) -----------------------------------------------
    def state_dict(self):
        """Optimiser state in ``torch.optim.AdamW.state_dict()`` layout (per-parameter ``step`` / ``exp_avg`` /
        ``exp_avg_sq`` in ``model.parameters()`` order, one param group) so that a reference-side resume can load it,
        plus this harness's own counters under ``"cgen"``."""
        eng, a = self.eng, self.args
        st = self.state.cpu()
        steps = float(st[OPT_STEPS])
        state = {}
        for i, p in enumerate(eng.params):
            o, k = eng.p_off[id(p)], p.numel()
            state[i] = {"step": torch.tensor(steps), "exp_avg": self.m[o:o + k].view(p.shape).clone(),
                        "exp_avg_sq": self.v[o:o + k].view(p.shape).clone()}
        group = {"lr": float(a.lr) * linear_warmup(int(a.lr_warmup_steps))(int(steps)), "betas": tuple(float(b) for b in a.betas),
                 "eps": 1e-8, "weight_decay": float(a.wd), "amsgrad": False, "maximize": False, "foreach": None, "capturable": False,
                 "differentiable": False, "fused": None, "initial_lr": float(a.lr), "params": list(range(len(eng.params)))}
        return {"state": state, "param_groups": [group],
                "cgen": {"it": self.it, "opt_steps": int(steps), "n_skipped": int(st[N_SKIPPED]),
                         "loss_scale_shift": int(self.eng.loss_scale_shift), "overflow_backoffs": int(self.overflow_backoffs),
                         "ls_growth_interval": int(self.ls_growth_interval),
                         "acc_g": None if self.acc_g is None else self.acc_g.clone()}}

    def scheduler_state_dict(self):
        """``LambdaLR.state_dict()`` of the reference's warm-up scheduler (train_setup.py:49-51): one step per successful
        optimiser step."""
        steps = int(self.state[OPT_STEPS].item())
        a = self.args
        lr = float(a.lr) * linear_warmup(int(a.lr_warmup_steps))(steps)
        return {"base_lrs": [float(a.lr)], "last_epoch": steps, "_step_count": steps + 1, "_get_lr_called_within_step": False,
                "_last_lr": [lr], "lr_lambdas": [None]}

    def load_state_dict(self, sd):
        """Inverse of :meth:`state_dict`; also accepts a plain ``torch.optim.AdamW`` state dict saved by the reference
        (the step count is then the parameters' common ``step``)."""
        eng = self.eng
        steps = None
        for i, p in enumerate(eng.params):
            ent = sd["state"].get(i)
            if ent is None:
                continue
            o, k = eng.p_off[id(p)], p.numel()
            self.m[o:o + k].copy_(ent["exp_avg"].reshape(-1))
            self.v[o:o + k].copy_(ent["exp_avg_sq"].reshape(-1))
            steps = float(ent["step"])
        extra = sd.get("cgen") or {}
        if "opt_steps" in extra:
            steps = float(extra["opt_steps"])
        st = torch.zeros(STATE_FLOATS)
        st[OPT_STEPS] = 0.0 if steps is None else steps
        st[N_SKIPPED] = float(extra.get("n_skipped", 0))
        self.state.copy_(st)
        self.it = int(extra.get("it", st[OPT_STEPS]))
        self._ls_checked_it, self._clean_checks, self._ls_last_growth_it = self.it, 0, None
        self._ls_nonfinite_seen = 0.0  # (state[N_NONFINITE] restarts at zero with the state vector)
        self.overflow_backoffs = int(extra.get("overflow_backoffs", 0))
        self.ls_growth_interval = int(extra.get("ls_growth_interval", self.ls_growth_interval))
        shift = max(self.LS_SHIFT_MIN, min(0, int(extra.get("loss_scale_shift", 0))))
        if shift != self.eng.loss_scale_shift:
            self._rescale(shift - self.eng.loss_scale_shift)
        if self.acc_g is not None and extra.get("acc_g") is not None:
            self.acc_g.copy_(extra["acc_g"])

    def _loss_scale_check(self):
        """Every `ls_check_interval` iterations (f16 engine only): one host read of the device step state.  A step since the
        previous check was dropped for a NON-FINITE gradient norm => an activation gradient left binary16's range: halve the scale (captured graphs
        and coefficient tables are rebuilt at this step) instead of dropping every later step as well.  After
        `ls_growth_interval` clean checks the scale is doubled back towards the rule's value; a growth that overflows again
        within one interval doubles that interval (no flapping).  The shift is clamped to [LS_SHIFT_MIN, 0]."""
        if self.eng.dtype_name == "f32" or self.it == 0 or self.it % self.ls_check_interval or self._ls_checked_it == self.it:
            return
        self._ls_checked_it = self.it
        s = self.state.cpu().tolist()
        # decided from a COUNTER, not from a sample of the last step: state[N_NONFINITE] counts the steps dropped for a non-finite
        # norm; any of the ls_check_interval steps since the previous check having overflowed backs the scale off, and a check only
        # counts as clean when none did
        overflow = s[N_NONFINITE] > self._ls_nonfinite_seen
        self._ls_nonfinite_seen = s[N_NONFINITE]
        if overflow:
            if self.eng.loss_scale_shift > self.LS_SHIFT_MIN:
                self._rescale(-1)
                self.overflow_backoffs += 1
            if self._ls_last_growth_it is not None and self.it - self._ls_last_growth_it <= self.ls_growth_interval * self.ls_check_interval:
                self.ls_growth_interval = min(4096, 2 * self.ls_growth_interval)
            self._ls_last_growth_it = None
            self._clean_checks = 0
        else:
            self._clean_checks += 1
            if self.eng.loss_scale_shift < 0 and self._clean_checks >= self.ls_growth_interval:
                self._rescale(+1)
                self._clean_checks = 0
                self._ls_last_growth_it = self.it

    def stats(self):
        """Host read of the device-side step state (one sync; call every N steps, not every step).  Read-only: the f16
        loss-scale back-off lives in step() (`_loss_scale_check`); `overflow_backoffs` counts the halvings so far,
        `loss_scale_shift` is the current log2 offset from the rule's value."""
        out = self.tail.stats()
        if self.eng.dtype_name != "f32":
            out.update(loss_scale=self.eng.loss_scale, loss_scale_shift=self.eng.loss_scale_shift, overflow_backoffs=self.overflow_backoffs)
        return out

    def _rescale(self, d):
        """Move the loss-scale back-off by `d` powers of two: everything that baked the old scale in is dropped (the captured
        step graphs, the seed coefficients, the engine's reduce tables are keyed by the scale)."""
        self.eng.loss_scale_shift = max(self.LS_SHIFT_MIN, min(0, self.eng.loss_scale_shift + d))
        torch.cuda.synchronize()
        self.graphs.clear()
        for ent in self.coefs.values():
            ent[1] = None
