"""Pair launches of the backward pass: a data-gradient launch is HELD until a partner reaches its own launch point, then the two
share one launch (cgen_block3_pair / cgen_block4_pair / cgen_conv2d_pair) or go out one after the other.  One `PairSlot` per
kernel family; `may_pair` is backward()'s rule for arming a fused Block's slot.  Host logic only (no torch, no library):
tests/test_pairing.py drives it with fakes.  DESIGN.md, "Pair launch"."""
from collections import namedtuple

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
