"""The forward pair slot (causal_gen_amd/pairing.py, HVAE._decode) without a GPU: the slot with fake launch functions, the decoder
loop on a fake engine (which layers pair, in which order the launches go out, that nothing stays held), the served-or-not decision
per layer for every preset, and the kernel's host-side answers for the shapes and the declined cases of the GPU test."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import fwd_pair_cases as fc
from causal_gen_amd import _lib, hps, vae
from causal_gen_amd.pairing import PairSlot


# ----------------------------------------------------------------------------- the slot, as Engine._block3_fwd drives it
def _slot(supported=True, prof=None):
    ev = []
    eng = SimpleNamespace(launches=10, prof=prof)

    def single(a, info):
        assert info == "info-" + a
        eng.launches += 1  # (as Engine._timed does)
        ev.append("single(%s)" % a)

    return PairSlot(eng, single, lambda h, a: ev.append("pair(%s,%s)" % (h, a)), lambda h, a: supported), eng, ev


def _submit(slot, a, writes, reads):
    slot.submit(a, set(writes), set(reads), "info-" + a)


POST = ("post", {"out_q", "mid_q"}, {"h", "pa", "acts"})
PRIOR = ("prior", {"out_p", "mid_p"}, {"z", "pa"})


def test_posterior_and_prior_share_one_launch():
    slot, eng, ev = _slot()
    slot.arm()
    _submit(slot, *POST)
    assert ev == [] and eng.launches == 10 and slot.held is not None
    _submit(slot, *PRIOR)  # (both read the parents)
    assert ev == ["pair(post,prior)"] and eng.launches == 11 and slot.pairs == 1 and not slot.busy


def test_a_launch_in_between_sends_two_singles_in_the_original_order():
    slot, eng, ev = _slot()
    slot.arm()
    _submit(slot, *POST)
    eng.launches += 1  # (an upsample, a lazily built parameter image ...)
    _submit(slot, *PRIOR)
    assert ev == ["single(post)", "single(prior)"] and eng.launches == 13 and slot.pairs == 0 and not slot.busy


@pytest.mark.parametrize("writes,reads", [({"out_p", "h"}, {"z"}), ({"out_p"}, {"z", "out_q"}), ({"out_q"}, {"z"})],
                         ids=["prior-writes-a-posterior-input", "prior-reads-the-posterior-output", "same-output"])
def test_overlapping_tensors_send_two_singles(writes, reads):
    slot, eng, ev = _slot()
    slot.arm()
    _submit(slot, *POST)
    _submit(slot, "prior", writes, reads)
    assert ev == ["single(post)", "single(prior)"] and slot.pairs == 0 and not slot.busy


def test_a_declined_pair_sends_two_singles():
    slot, eng, ev = _slot(supported=False)
    slot.arm()
    _submit(slot, *POST)
    _submit(slot, *PRIOR)
    assert ev == ["single(post)", "single(prior)"] and eng.launches == 12 and slot.pairs == 0 and not slot.busy


def test_nothing_is_held_in_a_profiled_pass():
    slot, eng, ev = _slot(prof={})
    slot.arm()
    _submit(slot, *POST)
    assert ev == ["single(post)"] and slot.held is None
    _submit(slot, *PRIOR)
    assert ev == ["single(post)", "single(prior)"] and slot.pairs == 0


def test_an_unarmed_slot_is_a_plain_launch():
    slot, eng, ev = _slot()
    _submit(slot, *POST)
    assert ev == ["single(post)"] and not slot.busy


# ----------------------------------------------------------------------------- HVAE._decode on a fake engine
class _T:
    """A tensor handle as _decode sees it: shape, channel views, crops."""

    def __init__(self, n, h, c, name):
        self.n, self.h, self.w, self.c, self.name, self.base, self.rg = n, h, h, c, name, self, True

    shape = property(lambda s: (s.n, s.h, s.w, s.c))

    def chan(self, a, b):
        v = _T(self.n, self.h, b - a, self.name)
        v.base = self.base
        return v

    def crop(self, r):
        return _T(self.n, r, self.c, self.name)


class _Eng:
    """The engine calls of a recorded decoder pass: a log of launches with the stream they went to, and the real PairSlot."""

    def __init__(self, supported=True, prof=None, gap=False, serial=False):
        self.launches, self.log, self.tape, self.prof, self.gap, self.blk3_fwd_pair_serial = 0, [], [], prof, gap, serial
        self.recording, self.infer_branch, self.fwd_branch, self.fwd_mainfirst = True, True, True, True
        self.side, self._bw_tag, self._fwd_pair_ok = False, 0, {}
        self._blk3f = PairSlot(self, lambda a, info: self._launch("block(%s)" % a),
                               lambda h, a: self.log.append("PAIR(%s,%s)" % (h, a)), lambda h, a: supported)

    def _launch(self, what):
        self.launches += 1
        self.log.append(what + ("@side" if self.side else ""))

    def block(self, name, res, fused):
        if fused:
            self._blk3f.submit(name, {name + ".out"}, {name + ".in"}, None)
        else:
            self._launch("convs(%s)" % name)
        self.tape.append((name, self._bw_tag))

    def bcast(self, p, B):
        return _T(B, 1, p.shape[1], "bias")

    def param_nhwc(self, p):
        pass

    def upsample(self, x, res, bp):
        self._launch("upsample")
        return _T(x.n, res, x.c, "up")

    def fork_mark(self):
        return None if self.prof is not None else "mark"

    def fork_side(self, after=None):
        if self.prof is not None:
            return False
        self.log.append("FORK")
        return True

    def on_side(self, fn, bw=0):
        old, self.side, old_tag, self._bw_tag = self.side, True, self._bw_tag, bw
        try:
            return fn()
        finally:
            self.side, self._bw_tag = old, old_tag

    def side_tagged(self, fn, bw=1):
        old_tag, self._bw_tag = self._bw_tag, bw
        try:
            return fn()
        finally:
            self._bw_tag = old_tag

    def join_side(self):
        self.log.append("JOIN")

    def latent_tail_fwd(self, site_p, site_f, q_loc, q_ls, p_loc, p_ls, p_feat, h, pa, eps, sid, logt, kptr, kstride, fb=None, tape_hold=None):
        self._launch("tail")
        return _T(h.n, h.h, q_loc.c, "z"), _T(h.n, h.h, h.c, "h"), _T(h.n, h.h, site_f, "zf") if site_f is not None else None


class _Host(vae._DecoderHost):
    def __init__(self, dec, fused_min_res):
        super().__init__(dec)
        self.fused_min_res = fused_min_res

    def _site(self, eng, conv):
        return conv.out_channels

    def _next_eps(self, eng, shape):
        return None

    def _scratch_kl(self, eng, B, res, zd):
        return 0

    def _run_block(self, eng, blk, segs):
        dec = self.decoder
        name = next("%s%d" % (k, i) for i, d in enumerate(dec.blocks) for k in ("prior", "posterior", "conv") if getattr(d, k, None) is blk)
        if eng.gap and name.startswith("prior"):
            eng._launch("fill")  # (something launched between the posterior Block's hold and the prior Block)
        eng.block(name, segs[0].h, fused=segs[0].h >= self.fused_min_res)
        return _T(segs[0].n, segs[0].h, blk.convs()[-1].out_channels, name)


def _decoder():
    hp = hps.setup_hparams("ukbb192", input_res=24, enc_arch="24b1d2,12b1d2,6b1d6,1b1", dec_arch="1b1,6b2,12b2", widths=[64, 96, 128],
                           z_max_res=12, z_dim=16, bs=3)
    hp.vr = "light"
    with torch.device("meta"):
        return vae.Decoder(hp), hp


def _decode(eng, pair_layers, monkeypatch):
    dec, hp = _decoder()
    monkeypatch.setattr(vae, "_lib", SimpleNamespace(load=lambda: SimpleNamespace(reparam_kl_chunks=lambda *a: 1)))
    for i in range(len(dec.blocks)):
        eng._fwd_pair_ok[(i, 3)] = i in pair_layers
    host = _Host(dec, fused_min_res=6)
    parents = _T(3, 12, hp.context_dim, "pa")
    parents.rg = False
    acts = {r: _T(3, r, 1, "act") for r in (1, 6, 12)}
    vae.HVAE._decode(host, eng, parents, acts=acts)
    return dec


# layers: 0 at 1 x 1 (unfused), 1 and 2 at 6 x 6, 3 and 4 at 12 x 12
def test_decode_pairs_the_armed_layers_and_forks_the_others_as_before(monkeypatch):
    eng = _Eng()
    _decode(eng, {1, 2, 3}, monkeypatch)
    assert eng.log == [
        # layer 0 forks (its Blocks are two conv launches each); nothing is forked ahead for layer 1, which pairs
        "convs(posterior0)", "FORK", "convs(prior0)@side", "JOIN", "tail", "convs(conv0)",
        # layer 1: both upsamples on the main stream, then ONE launch, no fork, no join
        "upsample", "upsample", "PAIR(posterior1,prior1)", "tail", "block(conv1)",
        "PAIR(posterior2,prior2)", "tail", "block(conv2)",
        # layer 4 does not pair: layer 3, which does, forks ahead for it behind its own tail, as an unpaired layer would
        "upsample", "upsample", "PAIR(posterior3,prior3)", "tail", "block(conv3)", "FORK",
        "block(prior4)@side", "block(posterior4)", "JOIN", "tail", "block(conv4)"], eng.log
    assert eng._blk3f.pairs == 3 and not eng._blk3f.busy
    # the tape: [prior][posterior] per layer with the prior tagged as a side-strand op, paired or not
    order = [e for e in eng.tape if not e[0].startswith("conv")]
    assert order == [(k + str(i), t) for i in range(5) for k, t in (("prior", 1), ("posterior", 0))], order


def test_a_pass_that_pairs_forks_nowhere_by_default(monkeypatch):
    """CGEN_BLK3_FWD_PAIR_SERIAL (the default): the layers the pair does not serve run prior Block, then posterior Block, in line."""
    eng = _Eng(serial=True)
    _decode(eng, {1, 2, 3}, monkeypatch)
    assert eng.log == [
        "convs(prior0)", "convs(posterior0)", "tail", "convs(conv0)",
        "upsample", "upsample", "PAIR(posterior1,prior1)", "tail", "block(conv1)",
        "PAIR(posterior2,prior2)", "tail", "block(conv2)",
        "upsample", "upsample", "PAIR(posterior3,prior3)", "tail", "block(conv3)",
        "block(prior4)", "block(posterior4)", "tail", "block(conv4)"], eng.log
    assert eng._blk3f.pairs == 3 and not eng._blk3f.busy
    order = [e[0] for e in eng.tape if not e[0].startswith("conv")]
    assert order == [k + str(i) for i in range(5) for k in ("prior", "posterior")], order


@pytest.mark.parametrize("serial", [False, True])
def test_decode_with_the_knob_off_is_the_two_queue_path(monkeypatch, serial):
    eng = _Eng(serial=serial)
    _decode(eng, set(), monkeypatch)
    assert not any(e.startswith("PAIR") for e in eng.log) and eng.log.count("FORK") == 5 and eng.log.count("JOIN") == 5
    assert eng.log.count("upsample@side") == 2 and eng._blk3f.pairs == 0 and not eng._blk3f.busy


@pytest.mark.parametrize("kw", [dict(supported=False), dict(gap=True)], ids=["declined-at-the-launch-point", "a-launch-in-between"])
def test_decode_falls_back_to_two_singles_on_the_main_stream(monkeypatch, kw):
    eng = _Eng(**kw)
    _decode(eng, {1}, monkeypatch)
    k = eng.log.index("block(posterior1)")
    assert eng.log[k:k + 2] == ["block(posterior1)", "block(prior1)"] and "FORK" not in eng.log[k - 3:k + 3], eng.log
    assert eng._blk3f.pairs == 0 and not eng._blk3f.busy


def test_decode_holds_nothing_in_a_profiled_pass(monkeypatch):
    eng = _Eng(prof={})
    _decode(eng, {1, 2, 3, 4}, monkeypatch)
    assert not any(e.startswith("PAIR") or e in ("FORK", "JOIN") for e in eng.log) and not eng._blk3f.busy


def test_an_exception_inside_a_paired_layer_leaves_the_slot_idle(monkeypatch):
    eng = _Eng()

    def boom(fn, bw=1):
        raise RuntimeError("prior Block failed")

    eng.side_tagged = boom
    with pytest.raises(RuntimeError):
        _decode(eng, {1}, monkeypatch)
    assert not eng._blk3f.busy


# ----------------------------------------------------------------------------- the decision, per layer of every preset
def _knobs(**over):
    d = dict(blk3_fwd_pair=1, f16=True, blk3_on=2, blk3_small=1, blk3_minres=16, blk3_res=[(20, 64)], blk3_res3=[(20, 112)],
             blk3_fwd_pair_res=[(4, 64)], blk3_fwd_pair_first=24, blk3_fwd_pair_serial=False, lib=_lib.load())
    d.update(over)
    return SimpleNamespace(**d)


def _served(name, B, **over):
    hp = hps.setup_hparams(name)
    with torch.device("meta"):
        m = vae.HVAE(hp)
    eng = _knobs(**over)
    return [(blk.res, vae.fwd_pair_layer(eng, m.decoder, i, B)) for i, blk in enumerate(m.decoder.blocks)]


@pytest.mark.parametrize("B", [32, 16, 3])
def test_ukbb192_pairs_its_layers_from_6_to_48_except_the_first_at_48(B):
    got = _served("ukbb192", B)
    want, seen = [], set()
    for res, _ in got:
        first = res not in seen
        seen.add(res)
        want.append((res, res in (6, 12, 24) or (res == 48 and not first)))
    assert got == want and sum(ok for _, ok in got) == 31


def test_the_first_layer_knob_and_the_range_knob():
    assert sum(ok for _, ok in _served("ukbb192", 32, blk3_fwd_pair_first=48)) == 32
    # a pass that forks nowhere (the default) has nothing to hide the first layer's upsample under: all 32 layers from 6 to 48 pair
    assert sum(ok for _, ok in _served("ukbb192", 32, blk3_fwd_pair_serial=True)) == 32
    assert {r for r, ok in _served("ukbb192", 32, blk3_fwd_pair_res=[(4, 12)]) if ok} == {6, 12}


@pytest.mark.parametrize("over", [dict(blk3_fwd_pair=0), dict(f16=False), dict(blk3_on=0)], ids=["knob-off", "f32-engine", "no-fused-block"])
def test_no_layer_pairs_without_the_knob_the_f16_engine_or_the_fused_block(over):
    assert not any(ok for _, ok in _served("ukbb192", 32, **over))


@pytest.mark.parametrize("name", [n for n in hps.HPARAMS_REGISTRY if n != "ukbb192"])
def test_presets_with_the_four_conv_block_pair_nothing(name):
    hp = hps.setup_hparams(name)
    assert not any(ok for _, ok in _served(name, hp.bs))


def test_q_correction_layers_do_not_pair():
    hp = hps.setup_hparams("ukbb192", q_correction=True)
    with torch.device("meta"):
        m = vae.HVAE(hp)
    assert not any(vae.fwd_pair_layer(_knobs(), m.decoder, i, 32) for i in range(len(m.decoder.blocks)))


# ----------------------------------------------------------------------------- the kernel's host-side answers (no GPU)
@pytest.mark.parametrize("shape", fc.SHAPES, ids=[s.name for s in fc.SHAPES])
def test_the_planner_gives_the_gpu_tests_shapes_their_instances(shape):
    lib = _lib.load()
    ok, plan = fc.plan(lib, fc.args(shape.n, shape.h, shape.w, shape.a), fc.args(shape.n, shape.h, shape.w, shape.b))
    assert ok == 1 and plan == shape.plan, plan


def test_no_smaller_shape_gives_the_two_records_different_tile_rows():
    lib = _lib.load()
    s = next(s for s in fc.SHAPES if s.name.startswith("nb3-th12"))
    best = None
    for n in range(1, 5):
        for h in range(8, 49, 4):
            for w in range(16, 2049, 16):
                if best is not None and n * h * w >= best[0]:
                    break
                ok, plan = fc.plan(lib, fc.args(n, h, w, s.a), fc.args(n, h, w, s.b))
                if ok and plan[3] != plan[6]:
                    best = (n * h * w, n, h, w)
                    break
    assert best == (s.n * s.h * s.w, s.n, s.h, s.w), best


def test_declined_combinations_answer_zero_without_a_gpu():
    lib = _lib.load()
    s = fc.SHAPES[0]
    a, b = fc.args(s.n, s.h, s.w, s.a), fc.args(s.n, s.h, s.w, s.b)
    assert lib.block3_pair_supported(C.byref(a), C.byref(b)) == 1
    cases = fc.declined(s.n, s.h, s.w, s.a, s.b) + [("row-streaming",) + fc.row_streaming()]
    assert len(cases) == 15
    for name, a, b in cases:
        assert lib.block3_supported(C.byref(a)) and lib.block3_supported(C.byref(b)), name  # (each record alone is served)
        assert lib.block3_pair_supported(C.byref(a), C.byref(b)) == 0, name
        assert lib.block3_pair_plan(C.byref(a), C.byref(b), None) == 0, name


def test_the_backward_pair_answers_what_it_answered():
    """Two data-gradient records of one instance are served as before; of different bottlenecks they are not."""
    lib = _lib.load()

    def dgrad(b, co):
        a = fc.args(8, 24, 24, fc.Rec([160], b, co), pre_act=0)
        a.mid_aux = a.mid
        a.o[0].aux = a.o[0].out
        a.bias_a = None
        a.o[0].bias = None
        return a

    assert lib.block3_pair_supported(C.byref(dgrad(32, 128)), C.byref(dgrad(32, 128))) == 1
    assert lib.block3_pair_supported(C.byref(dgrad(32, 128)), C.byref(dgrad(24, 128))) == 0
