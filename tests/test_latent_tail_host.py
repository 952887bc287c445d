"""The host side of a decoder layer's latent tail (causal_gen_amd/latent_tail.py) without a launch and without a GPU, on an Engine made
with __new__ whose library, allocator and gradient bookkeeping hooks are stubs that log what they are asked:

- Engine._latent_tail_at on hand-built tapes: both forms of the pattern -- stochastic (a reparam entry in front of z_proj, z its own
  tensor) and deterministic (no reparam entry, z_proj reading the slice [0, Z) of the prior Block's output) -- are recognised with and
  without z_feat_proj, and near misses are not;
- Engine.latent_tail_fwd and Engine._bw_latent_tail, both forms: a declined probe changes nothing; a served layer allocates, launches
  and records in the order of the separate launches, with exactly the absent views, the tape tags and the counter of its form.

The expectations are the table of differences at the head of latent_tail.py, written out; none is a recorded output."""
from types import SimpleNamespace

import pytest

Z, CW, CTX = 16, 32, 4
VIEWS_FWD = ("q_loc", "q_ls", "p_loc", "p_ls", "p_feat", "h_in", "pa", "eps", "z", "h_out", "zf")
VIEWS_BWD = ("g_h", "g_f", "gz_in", "q_loc", "q_ls", "p_loc", "p_ls", "z", "out_p", "out_q")
COUNTERS = ("lat_tails", "lat_tails_fwd", "lat_tails_det", "lat_tails_det_fwd")


def _engine(det=True):
    from causal_gen_amd.engine import Engine

    eng = Engine.__new__(Engine)
    eng.tape, eng.lat_tail_det = [], det
    return eng


def _nt(c, rg=True, n=2, hw=64, ptr=0x10000):
    from causal_gen_amd.engine import NT

    return NT(ptr, n, hw, hw, c, hw * hw * c, hw * c, c, 2, rg=rg)


def _site(name, seg_c, seg_rg, ks=1, bias=None):
    conv = SimpleNamespace(weight=SimpleNamespace(requires_grad=True), bias=bias)
    return SimpleNamespace(ks=ks, co=CW, seg_c=seg_c, seg_rg=seg_rg, name=name, conv=conv, img_fwd=0x5000 + 16 * len(name),
                           img_dg=[0x6000 + 16 * len(name), 0x6800 + 16 * len(name)])


def _layer(eng, feat=True, ks=1, loc=(0, Z), res=(2 * Z, 2 * Z + CW), loc_base=None, stochastic=False, q_same_base=False, q_ls_at=Z,
           pb_c=2 * Z + CW, f_seg=None, z_other=False, n=2, hw=64):
    """The tape entries of one layer in forward order ([reparam], z_proj, [conv Block], z_feat_proj is inserted right behind z_proj)."""
    from causal_gen_amd.engine import ACT_NONE

    pout, h, pa = _nt(pb_c, n=n, hw=hw), _nt(CW, n=n, hw=hw), _nt(CTX, rg=False, n=n, hw=hw)
    p_loc = (loc_base if loc_base is not None else pout).chan(*loc)
    p_feat = pout.chan(*res)
    site_p = _site("z_proj", [Z, CTX], [True, False], ks=ks)
    site_f = _site("z_feat_proj", [Z, CW], [True, True])
    if stochastic:
        z, qout = _nt(Z, n=n, hw=hw), (pout if q_same_base else _nt(2 * Z, n=n, hw=hw))
        eng.tape.append((eng._bw_reparam, (qout.chan(0, Z), qout.chan(q_ls_at, q_ls_at + Z), pout.chan(0, Z), pout.chan(Z, 2 * Z), z, 0.25, None, None), 0))
        p_loc = z
    eng.tape.append((eng._bw_conv, (site_p, [_nt(Z, n=n, hw=hw) if z_other else p_loc, pa], ACT_NONE, _nt(CW, n=n, hw=hw), h, p_feat), 0))
    if feat:
        eng.tape.append((eng._bw_conv, (site_f, [p_loc, pout.chan(*f_seg) if f_seg else p_feat], ACT_NONE, _nt(CW, n=n, hw=hw), None, None), 0))
    return len(eng.tape) - 1


# ----------------------------------------------------------------------------- the recogniser
@pytest.mark.parametrize("feat", [True, False])
def test_the_deterministic_pattern_is_accepted(feat):
    eng = _engine()
    i = _layer(eng, feat)
    f, a, r = eng._latent_tail_at(i)
    assert r is None and a is eng.tape[i - 1 if feat else i][1] and (f is eng.tape[i][1] if feat else f is None)


def test_the_knob_turns_it_off():
    eng = _engine(det=False)
    assert eng._latent_tail_at(_layer(eng)) is None


@pytest.mark.parametrize("feat", [True, False])
@pytest.mark.parametrize("miss", ["other_base", "residual_slice", "ks3", "loc_offset"])
def test_near_misses_are_rejected(miss, feat):
    eng = _engine()
    kw = {"other_base": dict(loc_base=_nt(2 * Z + CW)),         # the first segment is a slice of another tensor
          "residual_slice": dict(res=(Z, Z + CW)),              # the residual is not [2Z, 2Z + C)
          "ks3": dict(ks=3),                                    # a 3x3 site
          "loc_offset": dict(loc=(Z, 2 * Z))}[miss]             # the first segment is not [0, Z)
    assert eng._latent_tail_at(_layer(eng, feat, **kw)) is None


def test_a_whole_tensor_as_first_segment_is_not_the_pattern():
    """A stochastic layer's z is a tensor of its own: without its reparam entry in front it is left to the separate launches."""
    eng = _engine()
    i = _layer(eng, stochastic=True)
    del eng.tape[i - 2]  # (the reparam entry)
    assert eng._latent_tail_at(i - 1) is None


@pytest.mark.parametrize("det_knob", [True, False])  # (the stochastic form does not ask lat_tail_det)
@pytest.mark.parametrize("feat", [True, False])
def test_the_stochastic_pattern_is_accepted(feat, det_knob):
    eng = _engine(det=det_knob)
    i = _layer(eng, feat, stochastic=True)
    f, a, r = eng._latent_tail_at(i)
    j = i - 1 if feat else i
    assert r is eng.tape[j - 1][1] and a is eng.tape[j][1] and (f is eng.tape[i][1] if feat else f is None)


def _stochastic_miss(kw, feat=True):
    eng = _engine()
    return eng._latent_tail_at(_layer(eng, feat, stochastic=True, **kw))


def test_stochastic_q_and_p_on_one_base_is_rejected():
    assert _stochastic_miss(dict(q_same_base=True)) is None


def test_stochastic_q_ls_not_at_offset_z_is_rejected():
    assert _stochastic_miss(dict(q_ls_at=0)) is None


def test_stochastic_prior_output_wider_than_2z_plus_c_is_rejected():
    assert _stochastic_miss(dict(pb_c=2 * Z + CW + 8)) is None


def test_stochastic_z_feat_proj_reading_another_slice_is_rejected():
    assert _stochastic_miss(dict(f_seg=(Z, Z + CW))) is None


@pytest.mark.parametrize("feat", [True, False])
def test_stochastic_3x3_site_is_rejected(feat):
    assert _stochastic_miss(dict(ks=3), feat) is None


def test_stochastic_z_proj_not_reading_the_reparams_z_is_rejected():
    assert _stochastic_miss(dict(z_other=True), feat=False) is None


# ----------------------------------------------------------------------------- forward and backward on a stub library
class _Lib:
    """Answers the two probes with `supported`, keeps a copy of every struct it is handed, logs every call."""

    def __init__(self, log, supported):
        self.log, self.supported, self.structs = log, supported, {}

    def _take(self, what, ref):
        self.log.append(what)
        self.structs[what] = type(ref._obj).from_buffer_copy(ref._obj)

    def latent_tail_fwd_supported(self, ref):
        self._take("fwd_supported", ref)
        return self.supported

    def latent_tail_bwd_supported(self, ref):
        self._take("bwd_supported", ref)
        return self.supported

    def latent_tail_fwd(self, ref, stream):
        self._take("fwd", ref)

    def latent_tail_bwd(self, ref, stream):
        self._take("bwd", ref)

    def kl_channel_sums(self, *a):
        self.log.append("kl_channel_sums")


def _stub_engine(supported=1):
    """An Engine that was never initialised: f16, recording, every latent-tail knob on, side-strand tag 1 (so the tag of an entry says
    whether it is _bw_tag or a literal 0); `new`, `new_f32`, `rng_ptr` hand out fake pointers, `_wgrad`, `_grad_residual` and
    `grad_write` log (grad_write then does its real bookkeeping).  Returns (engine, log)."""
    from causal_gen_amd.engine import F16, NT, Engine, _Tape

    eng, log, nxt = Engine.__new__(Engine), [], [0x100000]
    eng.lib, eng.dt, eng.es, eng.prof, eng._ablate, eng.stream, eng.launches = _Lib(log, supported), F16, 2, None, frozenset(), 0, 0
    eng.recording, eng.trunk_mode, eng.trunk_maxres, eng._bw_tag, eng._dbg_names, eng.kl_coef_override = True, 1, 100000, 1, None, None
    eng.tape = _Tape()
    eng.tape.eng = eng
    eng.lat_tail = eng.lat_tail_fwd = eng.lat_tail_det = True
    eng.lat_tail_minpx = eng.lat_tail_fwd_minpx = 0
    eng.lat_tail_exact = False
    for k in COUNTERS:
        setattr(eng, k, 0)
    eng.grads, eng._riders, eng._adopted, eng._wg_events, eng.wgrad_batch = {}, {}, set(), [], True
    eng.kl_coef_ptr, eng.kl_chan_ptr = 0x7000, 0x7800

    def new(n, h, w, c, rg=True, es=None, rem=False):
        log.append("new %d" % c)
        nxt[0] += 0x10000
        return NT(nxt[0], n, h, w, c, h * w * c, w * c, c, 2, rg=rg)

    def new_f32(count):
        log.append("new_f32 %d" % count)
        nxt[0] += 0x10000
        return nxt[0]

    def grad_write(t, defer_hazard=False):
        log.append("grad_write [%d, %d)" % (t.coff, t.coff + t.c))
        return Engine.grad_write(eng, t, defer_hazard)

    eng.new, eng.new_f32, eng.rng_ptr, eng.grad_write = new, new_f32, (lambda: 0x9000), grad_write
    eng._wgrad = lambda site, segs, act, g: log.append("wgrad " + site.name)
    eng._grad_residual = lambda r, g, out, segs: log.append("residual %d" % r.c)
    return eng, log


def _nulls(t, names):
    return {k for k in names if not getattr(t, k).p}


def _fwd(form, feat, supported=1, fb=None, eps=False):
    """Engine.latent_tail_fwd on a layer of 1 x 4 x 4 pixels.  Returns (engine, log, result, hold, the layer's tensors)."""
    eng, log = _stub_engine(supported)
    kw = dict(n=1, hw=4)
    pout, qout, h, pa = _nt(2 * Z + CW, ptr=0x20000, **kw), _nt(2 * Z, ptr=0x30000, **kw), _nt(CW, ptr=0x40000, **kw), _nt(CTX, rg=False, ptr=0x50000, **kw)
    x = SimpleNamespace(p_loc=pout.chan(0, Z), p_ls=pout.chan(Z, 2 * Z), p_feat=pout.chan(2 * Z, 2 * Z + CW), q_loc=qout.chan(0, Z),
                        q_ls=qout.chan(Z, 2 * Z), h=h, pa=pa, eps=_nt(Z, rg=False, ptr=0x60000, **kw) if eps else None,
                        site_p=_site("z_proj", [Z, CTX], [True, False], bias=SimpleNamespace(data_ptr=lambda: 0xB000)),
                        site_f=_site("z_feat_proj", [Z, CW], [True, True]) if feat else None)
    hold = []
    if form == "stochastic":
        out = eng.latent_tail_fwd(x.site_p, x.site_f, x.q_loc, x.q_ls, x.p_loc, x.p_ls, x.p_feat, h, pa, x.eps, 1003, 0.25, 0xA000, 2, fb=fb, tape_hold=hold)
    else:  # (as HVAE._decode calls it for such a layer: no q, but the prior Block's p_ls, the pass's stream id and temperature)
        out = eng.latent_tail_fwd(x.site_p, x.site_f, None, None, x.p_loc, x.p_ls, x.p_feat, h, pa, None, 1003, 0.25, None, None, fb=None, tape_hold=hold)
    return eng, log, out, hold, x


@pytest.mark.parametrize("feat", [True, False])
@pytest.mark.parametrize("form", ["stochastic", "deterministic"])
def test_forward_declined_does_nothing(form, feat):
    eng, log, out, hold, _ = _fwd(form, feat, supported=0, fb=(0xC000, 64, 8))
    assert out is None and log == ["fwd_supported"]  # (nothing allocated, no launch of any kind)
    assert list(eng.tape) == [] and hold == [] and eng.launches == 0 and all(getattr(eng, k) == 0 for k in COUNTERS)


@pytest.mark.parametrize("eps", [False, True])
@pytest.mark.parametrize("fb", [None, (0xC000, 64, 8)])
@pytest.mark.parametrize("feat", [True, False])
def test_forward_stochastic_served(feat, fb, eps):
    from causal_gen_amd.engine import ACT_NONE

    eng, log, (z, h2, zf), hold, x = _fwd("stochastic", feat, fb=fb, eps=eps)
    # new(z), kl_channel_sums only with free bits (a launch, counted), new(h'), new(zf), the launch
    assert log == ["fwd_supported", "new %d" % Z] + ["kl_channel_sums"] * (fb is not None) + ["new %d" % CW] * (2 if feat else 1) + ["fwd"]
    assert eng.launches == (2 if fb is not None else 1)
    t = eng.lib.structs["fwd"]
    assert _nulls(t, VIEWS_FWD) == ({"eps"} if not eps else set()) | ({"zf"} if not feat else set())  # only eps (and an absent zf) may be NULL
    assert (t.z.p, t.h_out.p, t.zf.p) == (z.ptr, h2.ptr, zf.ptr if feat else None) and (zf is None) == (not feat)
    assert (t.q_loc.p, t.q_ls.p, t.p_loc.p, t.p_ls.p, t.p_feat.p) == (x.q_loc.ptr, x.q_ls.ptr, x.p_loc.ptr, x.p_ls.ptr, x.p_feat.ptr)
    assert (t.n, t.h, t.w, t.z_dim, t.c, t.ctx) == (1, 4, 4, Z, CW, CTX) and (t.h_in.p, t.pa.p) == (x.h.ptr, x.pa.ptr)
    assert (t.kl_stride, t.stream_id, t.logt, t.rng, t.kl_part) == (2, 1003, 0.25, 0x9000, 0xA000)  # the fields of this form alone
    assert (t.img_p, t.img_f, t.bias_p, t.bias_f) == (x.site_p.img_fwd, x.site_f.img_fwd if feat else None, 0xB000, None)
    # tape: reparam, z_proj (tag _bw_tag = 1); z_feat_proj into tape_hold with tag 0
    assert list(eng.tape) == [(eng._bw_reparam, (x.q_loc, x.q_ls, x.p_loc, x.p_ls, z, 0.25, None if fb is None else 8, None), 1),
                              (eng._bw_conv, (x.site_p, [z, x.pa], ACT_NONE, h2, x.h, x.p_feat), 1)]
    assert hold == ([(eng._bw_conv, (x.site_f, [z, x.p_feat], ACT_NONE, zf, None, None), 0)] if feat else [])
    assert {k: getattr(eng, k) for k in COUNTERS} == dict(lat_tails=0, lat_tails_fwd=1, lat_tails_det=0, lat_tails_det_fwd=0)


@pytest.mark.parametrize("feat", [True, False])
def test_forward_deterministic_served(feat):
    from causal_gen_amd.engine import ACT_NONE

    eng, log, (z, h2, zf), hold, x = _fwd("deterministic", feat)
    assert log == ["fwd_supported"] + ["new %d" % CW] * (2 if feat else 1) + ["fwd"] and eng.launches == 1  # new(h'), new(zf), the launch
    t = eng.lib.structs["fwd"]
    assert _nulls(t, VIEWS_FWD) == {"q_loc", "q_ls", "p_ls", "eps", "z"} | ({"zf"} if not feat else set())
    assert z is x.p_loc and (t.p_loc.p, t.p_feat.p, t.h_in.p, t.pa.p) == (x.p_loc.ptr, x.p_feat.ptr, x.h.ptr, x.pa.ptr)
    assert (t.h_out.p, t.zf.p) == (h2.ptr, zf.ptr if feat else None) and (t.n, t.h, t.w, t.z_dim, t.c, t.ctx) == (1, 4, 4, Z, CW, CTX)
    assert (t.kl_stride, t.stream_id, t.logt, t.rng, t.kl_part) == (0, 0, 0.0, None, None)  # never set in this form
    assert (t.img_p, t.img_f, t.bias_p, t.bias_f) == (x.site_p.img_fwd, x.site_f.img_fwd if feat else None, 0xB000, None)
    # tape: z_proj (tag _bw_tag = 1); z_feat_proj into tape_hold with tag _bw_tag
    assert list(eng.tape) == [(eng._bw_conv, (x.site_p, [x.p_loc, x.pa], ACT_NONE, h2, x.h, x.p_feat), 1)]
    assert hold == ([(eng._bw_conv, (x.site_f, [x.p_loc, x.p_feat], ACT_NONE, zf, None, None), 1)] if feat else [])
    assert {k: getattr(eng, k) for k in COUNTERS} == dict(lat_tails=0, lat_tails_fwd=0, lat_tails_det=0, lat_tails_det_fwd=1)


def test_forward_knobs_gate_their_own_form():
    """lat_tail_fwd and its pixel floor gate the stochastic form only, lat_tail_det the deterministic form only (no probe is made)."""
    for knob, value, declined in (("lat_tail_fwd", False, "stochastic"), ("lat_tail_fwd_minpx", 17, "stochastic"), ("lat_tail_det", False, "deterministic")):
        for form in ("stochastic", "deterministic"):
            eng, log = _stub_engine()
            setattr(eng, knob, value)
            kw = dict(n=1, hw=4)
            pout, qout = _nt(2 * Z + CW, **kw), _nt(2 * Z, **kw)
            q = (qout.chan(0, Z), qout.chan(Z, 2 * Z)) if form == "stochastic" else (None, None)
            out = eng.latent_tail_fwd(_site("z_proj", [Z, CTX], [True, False]), None, q[0], q[1], pout.chan(0, Z), pout.chan(Z, 2 * Z),
                                      pout.chan(2 * Z, 2 * Z + CW), _nt(CW, **kw), _nt(CTX, rg=False, **kw), None, 1, 0.0, 0xA000, 2)
            assert (out is None and log == []) if form == declined else out is not None, (knob, form)


def _bwd(form, feat, supported=1, have=None):
    """Engine._bw_latent_tail on what Engine._latent_tail_at finds on a hand-built tape; grad(h') and grad(zf) hold a value, `have`:
    intervals grad(pout) holds already.  Returns (engine, log, result, (f, a, r))."""
    eng, log = _stub_engine(supported)
    i = _layer(eng, feat, stochastic=form == "stochastic", n=1, hw=4)
    ents = eng._latent_tail_at(i)
    f, a, r = ents
    assert (r is None) == (form == "deterministic") and (f is None) == (not feat)
    for e in (a, f):
        if e is not None:
            eng.grads[id(e[3])] = [_nt(CW, rg=False, n=1, hw=4, ptr=0x70000), [(0, CW)], e[3]]
    if have:
        pb = a[5].base
        eng.grads[id(pb)] = [_nt(pb.c, rg=False, n=1, hw=4, ptr=0x80000), list(have), pb]
    del log[:]
    before = {k: list(e[1]) for k, e in eng.grads.items()}
    return eng, log, eng._bw_latent_tail(*ents), ents, before


@pytest.mark.parametrize("feat", [True, False])
@pytest.mark.parametrize("form", ["stochastic", "deterministic"])
def test_backward_declined_does_nothing(form, feat):
    """(The probe's output views come from _gentry, which makes the gradient buffers the separate launches' grad_write would make: a
    declined probe may leave such a buffer behind -- WITHOUT an interval, which is what says that a gradient holds a value.)"""
    eng, log, ok, _, before = _bwd(form, feat, supported=0)
    assert ok is False and [e for e in log if not e.startswith("new ")] == ["bwd_supported"]  # (no wgrad, no residual, no grad_write, no launch)
    assert {k: e[1] for k, e in eng.grads.items() if e[1]} == before and eng._wg_events == [] and eng._riders == {}
    assert eng.launches == 0 and all(getattr(eng, k) == 0 for k in COUNTERS)


@pytest.mark.parametrize("feat", [True, False])
@pytest.mark.parametrize("form", ["stochastic", "deterministic"])
def test_backward_served_runs_the_committed_block_in_order(form, feat):
    eng, log, ok, (f, a, r), _ = _bwd(form, feat)
    sto = form == "stochastic"
    # wgrad(z_feat_proj), the residuals other than p_feat (h), wgrad(z_proj), grad_write (p, then q), the launch
    assert ok is True and [e for e in log if not e.startswith("new ")] == (
        ["bwd_supported"] + ["wgrad z_feat_proj"] * feat + ["residual %d" % CW, "wgrad z_proj", "grad_write [0, %d)" % (2 * Z + CW)]
        + ["grad_write [0, %d)" % (2 * Z)] * sto + ["bwd"])
    t, pb = eng.lib.structs["bwd"], a[5].base
    absent = {"gz_in"} if sto else {"gz_in", "q_loc", "q_ls", "p_loc", "p_ls", "z", "out_q"}  # (nothing flowed into grad(z) here: gz_in NULL)
    assert _nulls(t, VIEWS_BWD) == absent | ({"g_f"} if not feat else set())
    assert (t.n, t.h, t.w, t.z_dim, t.c, t.parity, t.acc_p, t.acc_q) == (1, 4, 4, Z, CW, 1, 0, 0)
    assert t.out_p.p == eng.grads[id(pb)][0].ptr and eng.grads[id(pb)][1] == [(0, 2 * Z + CW)]  # the whole pixel of grad(pout), in one write
    assert (t.img_fz, t.img_fp, t.img_pz) == ((f[0].img_dg[0], f[0].img_dg[1]) if feat else (None, None)) + (a[0].img_dg[0],)
    if sto:
        qb = r[0].base
        assert t.out_q.p == eng.grads[id(qb)][0].ptr and eng.grads[id(qb)][1] == [(0, 2 * Z)]
        assert (t.coef, t.coef_stride, t.logt, t.chan_scale) == (0x7000, 0, 0.25, None)
        assert (t.q_loc.p, t.q_ls.p, t.p_loc.p, t.p_ls.p, t.z.p) == tuple(v.ptr for v in r[:5])
    else:
        assert (t.coef, t.coef_stride, t.logt, t.chan_scale) == (None, 0, 0.0, None)  # never set in this form
    assert eng.launches == 1 and eng._wg_events == []
    assert {k: getattr(eng, k) for k in COUNTERS} == dict(lat_tails=int(sto), lat_tails_fwd=0, lat_tails_det=int(not sto), lat_tails_det_fwd=0)


@pytest.mark.parametrize("have", [[(0, Z)], [(Z, 2 * Z)], [(2 * Z, 2 * Z + CW)], [(0, 2 * Z + CW)]], ids=["p_loc", "p_ls", "p_feat", "all"])
def test_backward_deterministic_declines_a_gradient_that_holds_a_value(have):
    """The deterministic kernels do not accumulate: any interval of [0, 2Z + C) in grad(pout) sends the layer to the separate launches."""
    eng, log, ok, _, before = _bwd("deterministic", True, have=have)
    assert ok is False and log == [] and {k: e[1] for k, e in eng.grads.items()} == before
    assert eng.launches == 0 and all(getattr(eng, k) == 0 for k in COUNTERS)


def test_backward_stochastic_accumulates_into_a_gradient_that_holds_a_value():
    eng, log, ok, (f, a, r), _ = _bwd("stochastic", True, have=[(0, 2 * Z + CW)])
    t = eng.lib.structs["bwd"]
    assert ok is True and (t.acc_p, t.acc_q) == (1, 0) and eng.lat_tails == 1


def test_backward_pixel_floor_is_the_stochastic_forms():
    for form in ("stochastic", "deterministic"):
        eng, log = _stub_engine()
        eng.lat_tail_minpx = 17  # (the layer has 16 pixels)
        i = _layer(eng, True, stochastic=form == "stochastic", n=1, hw=4)
        ents = eng._latent_tail_at(i)
        for e in ents[:2]:
            eng.grads[id(e[3])] = [_nt(CW, rg=False, n=1, hw=4, ptr=0x70000), [(0, CW)], e[3]]
        assert eng._bw_latent_tail(*ents) is (form == "deterministic"), form
