"""Pair launches: a launch is HELD until a partner reaches its own launch point, then the two share one launch (cgen_block3_pair /
cgen_block4_pair / cgen_conv2d_pair) or go out one after the other.  One `PairSlot` per kernel family and direction; `may_pair` is
backward()'s rule for arming a fused Block's slot, `fwd_pair_expected` the decoder's rule for a layer's posterior and prior Blocks
in the forward pass.  Host logic only (no torch; the library only through the `lib` handed in): tests/test_pairing.py and
tests/test_pairing_fwd.py drive it with fakes.  DESIGN.md, "Pair launch"."""
import ctypes as C
from collections import namedtuple

FwdBlock = namedtuple("FwdBlock", "light nconv residual down seg_c b co")  # what the rule needs to know of a Block (vae.Block)

# args of a fused Block's tape entry (fn, args, tag); fn(*args) is its backward.  `mids`: the bottleneck tensors.
BlockRec = namedtuple("BlockRec", "sites segs mids out res1")


def _nothing():
    pass


def may_pair(entry, nxt):
    """Tape entry `entry` (a fused Block, the one backward() is about to run) may wait for `nxt` (the entry that runs after it, or
    None): the same kind of fused Block on the same image size without a residual -- a decoder layer's prior Block behind its
    posterior Block -- that reads none of this Block's differentiable inputs (else its bookkeeping, an accumulate target or a
    copy-on-write of the shared gradient, could launch work that must see this Block's result first) nor this Block's inputs as
    its output."""
    if nxt is None or nxt[0] != entry[0]:
        return False
    a, b = entry[1], nxt[1]
    return (b.res1 is None and (b.segs[0].h, b.segs[0].w) == (a.segs[0].h, a.segs[0].w)
            and not ({id(v.base) for v in a.segs if v.rg} & {id(v.base) for v in b.segs if v.rg})
            and not any(v.base is b.out.base for v in a.segs))


class PairSlot:
    """idle -> armed (`arm`: the next submitted launch is to be held) -> holding (`held`: it waits for its partner).

    `eng` supplies `launches` (the launch counter: a pair needs it unchanged since the hold, i.e. nothing was enqueued between the
    two) and `prof` (profiling: never hold).  `single(args, info)` launches one problem alone (and counts it), `pair(held_args,
    args)` launches two (the slot counts that one, and in `pairs`), `supported(held_args, args)` is the family's *_pair_supported."""

    def __init__(self, eng, single, pair, supported):
        self.eng, self._single, self._pair, self._supported = eng, single, pair, supported
        self.armed, self.held, self.pairs = False, None, 0

    @property
    def busy(self):
        return self.armed or self.held is not None

    def reset(self):
        """Back to idle; a held launch is dropped (the pass that held it died in an exception)."""
        self.armed, self.held = False, None

    def arm(self):
        self.armed = True

    def disarm(self):
        """The armed launch did not reach its launch point.  (No effect on a held one.)"""
        self.armed = False

    def submit(self, args, writes, reads, info, late=_nothing):
        """A data-gradient launch at its launch point.  `writes` / `reads`: the tensors it touches (storage identity; a pair must
        not touch each other's).  `late`: bookkeeping that reads what the launch writes (the weight gradient of the Block's first
        conv); queued only BEHIND the launch, so that a background flush triggered in between cannot see it."""
        eng = self.eng
        if self.armed and eng.prof is None:
            self.held, self.armed = (args, eng.launches, writes, reads, info, late), False  # the partner launches both
            return
        if self.held is not None:
            hargs, hl, hwr, hrd, _, hlate = self.held
            if hl == eng.launches and not (hwr & (writes | reads)) and not (writes & hrd) and self._supported(hargs, args):
                self.reset()
                self._pair(hargs, args)
                eng.launches += 1
                self.pairs += 1
                hlate()
                late()
                return
            self.flush()
        self._single(args, info)
        late()

    def flush(self):
        """Disarm, and launch a held problem on its own (its partner did not come, or cannot share the launch)."""
        held = self.held
        self.reset()
        if held is not None:
            self._single(held[0], held[4])
            held[5]()


def _in_ranges(v, ranges):
    return not ranges or any(lo <= v <= hi for lo, hi in ranges)


def fwd_pair_expected(eng, libmod, n, res, first, post, prior):
    """Will the forward pass of a stochastic decoder layer at `res` x `res`, batch `n`, send its posterior Block `post` and its prior
    Block `prior` (FwdBlock each) as ONE launch?  Decided before the layer runs (the layer in front of it must know whether to fork a
    side stream ahead), from what is known then: the engine's dtype and knobs (`eng`: blk3_fwd_pair, blk3_fwd_pair_res,
    blk3_fwd_pair_first, blk3_fwd_pair_serial, blk3_on, blk3_small, blk3_minres, blk3_res, blk3_res3, f16, lib), the resolution and the widths.  `first`:
    the layer is the first of its resolution (its z is upsampled in front of the prior Block).  The kernel's own answer
    (cgen_block3_pair_supported, host code) is asked on dense stand-ins of the tensors; `libmod` is causal_gen_amd._lib (the
    argument records).  A wrong "yes" costs nothing but the pair: the slot sends the two launches singly."""
    if not (eng.blk3_fwd_pair and eng.f16 and eng.blk3_on and _in_ranges(res, eng.blk3_fwd_pair_res)):
        return False
    if first and res > eng.blk3_fwd_pair_first and not eng.blk3_fwd_pair_serial:
        return False  # (that layer keeps the fork, which hides the upsample; a pass that forks nowhere has nothing to hide it under)
    for blk in (post, prior):
        # Engine.block2's own conditions for the one-launch Block (the 1x1 layers and the four-conv Block never get there)
        if not (blk.light and blk.nconv == 2 and not blk.residual and not blk.down and blk.b % 8 == 0 and blk.co % 8 == 0
                and 1 <= len(blk.seg_c) <= 3):
            return False
        small = eng.blk3_small and res <= 14 and res >= 4
        res_ok = eng.blk3_res3 if len(blk.seg_c) >= 3 else eng.blk3_res
        tile_ok = res >= eng.blk3_minres and blk.b <= 32 and _in_ranges(res, res_ok)
        if not ((small and blk.b <= 64) or tile_ok):
            return False
    return bool(eng.lib.block3_pair_supported(C.byref(fwd_probe_args(libmod, n, res, post)), C.byref(fwd_probe_args(libmod, n, res, prior))))


def fwd_probe_args(libmod, n, res, blk, f16=1):
    """cgen_block3_args of a forward Block on dense stand-ins of its tensors (aligned, never dereferenced by the host-side planner);
    a segment whose width is no multiple of 8 stands for the parents: spatially constant, zero-padded to 8."""
    a = libmod.Block3Args()
    a.dtype, a.n, a.h, a.w, a.nseg, a.nout, a.pre_act = f16, n, res, res, len(blk.seg_c), 1, 1
    fake = 1 << 20

    def dense(c):
        cp = -(-c // 8) * 8
        if c % 8:
            return libmod.View(fake, cp, 0, 0, c, cp)
        return libmod.View(fake, res * res * cp, res * cp, cp, c, 0)

    for k, c in enumerate(blk.seg_c):
        a.seg[k] = dense(c)
    a.w_a, a.bias_a = fake, fake
    a.mid, a.mid_aux = dense(blk.b), libmod.NULL_VIEW
    o = a.o[0]
    o.w, o.bias, o.out, o.aux, o.res1 = fake, fake, dense(blk.co), libmod.NULL_VIEW, libmod.NULL_VIEW
    return a
