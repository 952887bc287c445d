"""Engine.like_head_fwd / _bw_like_head without a GPU: the two methods run on a stand-in engine whose library records every call.
What is checked is the launch sequence the engine issues in both settings of CGEN_LIKE_HEAD and the bookkeeping around it: one tape
entry, the two head sites registered as weight-gradient events in tape order AFTER the launch that writes their partials, their cost
added to the flush mark's running sum, nothing left in the deferred batch."""
import types
from types import SimpleNamespace

import torch


class StubLib:
    def __init__(self, served=1):
        self.calls, self.served = [], served

    def dgauss_head_supported(self, ref):
        self.calls.append(("dgauss_head_supported", None))
        return self.served

    def dgauss_head_fwd(self, ref, st):
        t = ref._obj
        self.calls.append(("dgauss_head_fwd", (t.params.p, t.params.c, t.params.sw, t.nll_part, t.img_loc, t.img_ls, st)))

    def dgauss_head_bwd(self, ref, st):
        t = ref._obj
        self.calls.append(("dgauss_head_bwd", (t.coef_dev, t.coef_stride, t.nsplit, t.g_h.p, t.g_params.p, t.partial_w_loc, t.partial_b_loc,
                                               t.partial_w_ls, t.partial_b_ls, st)))


def _site(name, index, img, train_w=True, bias=True, co=1, ks=1):
    conv = torch.nn.Conv2d(32, co, ks, bias=bias)
    conv.weight.requires_grad = train_w
    return SimpleNamespace(name=name, index=index, conv=conv, ks=ks, co=co, ci=32, taps=ks * ks, seg_c=[32], img_fwd=img)


def _engine(lib, knob=True, recording=True, dt=None, prof=None):
    from causal_gen_amd import engine as E

    eng = SimpleNamespace()
    eng.like_head, eng.recording, eng.dt, eng.prof, eng._ablate = knob, recording, (E.F16 if dt is None else dt), prof, set()
    eng.lib, eng.stream, eng.launches, eng.like_heads, eng._dbg_names, eng._bw_tag = lib, 77, 0, 0, None, 0
    eng.tape, eng.grads, eng.es = [], {}, 2
    eng._next = [0x10000]

    def new(n, h, w, c, rg=True):
        p = eng._next[0]
        eng._next[0] += n * h * w * 8 * 2
        return E.NT(p, n, h, w, c, h * w * 8, w * 8, 8, 2, rg=rg)

    def new_f32(count):
        p = eng._next[0]
        eng._next[0] += 4 * count
        return p

    eng.new, eng.new_f32 = new, new_f32
    for nm in ("like_head_fwd", "_bw_like_head", "_like_head_args"):
        setattr(eng, nm, types.MethodType(getattr(E.Engine, nm), eng))
    # backward bookkeeping
    eng.like_coef_ptr = 0xC0EF
    eng._wg_events, eng._wg_deferred, eng._wg_cum, eng.marks = [], [], 0.0, []
    eng._defer_wgrad = lambda: True
    eng._wgrad_marks = lambda: eng.marks.append((len(lib.calls), len(eng._wg_events), eng._wg_cum))
    eng._dgrad_target = lambda s: (new(s.n, s.h, s.w, s.c, rg=False), None, False)

    def plan(site, segs, act, g):
        a = SimpleNamespace(partial_w=0x5000 + 0x100 * site.index, partial_b=0x5080 + 0x100 * site.index)
        eng.plans.append((site.name, g.p, g.c, g.sw))
        return a, ("key", site.index), 25

    eng.plans, eng._wgrad_plan = [], plan
    return eng


def _tensors(eng):
    return eng.new(2, 56, 56, 32), eng.new(2, 56, 56, 1, rg=False)


def test_fused_path_issues_one_launch_each_way_and_registers_both_sites():
    lib = StubLib()
    eng = _engine(lib)
    loc, ls = _site("x_loc", 3, 0xA000), _site("x_logscale", 4, 0xB000)
    h, x = _tensors(eng)
    params, nll = eng.like_head_fwd(loc, ls, h, x, 8)
    assert [c[0] for c in lib.calls] == ["dgauss_head_supported", "dgauss_head_fwd"]
    assert lib.calls[1][1] == (params.ptr, 2, 8, nll, 0xA000, 0xB000, 77)
    assert nll == params.ptr + 2 * 56 * 56 * 8 * 2  # the partials follow the parameter tensor in the arena, as on the unfused path
    assert (params.c, eng.like_heads, eng.launches) == (2, 1, 0)  # (HVAE._elbo_pass counts this launch with elbo_finalize)
    assert len(eng.tape) == 1 and eng.tape[0][0] == eng._bw_like_head and eng.tape[0][1] == (loc, ls, h, params, x)
    # ---- backward of that entry
    fn, args, _ = eng.tape[0]
    fn(*args)
    assert [c[0] for c in lib.calls[2:]] == ["dgauss_head_bwd"]
    coef, stride, nsplit, gh, gparams, pwl, pbl, pws, pbs, st = lib.calls[2][1]
    assert (coef, stride, nsplit, st) == (0xC0EF, 0, 25, 77) and gh and not gparams  # grad(params) is never stored
    assert (pwl, pbl, pws, pbs) == (0x5300, 0x5380, 0x5400, 0x5480)
    # the plans were made for one-channel slices of the parameter tensor's layout, x_logscale (channel 1) first: the tape's order
    assert eng.plans == [("x_logscale", params.ptr + 2, 1, 8), ("x_loc", params.ptr, 1, 8)]
    assert [(s.name, k, n) for s, k, n in eng._wg_events] == [("x_logscale", ("key", 4), 25), ("x_loc", ("key", 3), 25)]
    cost = 2.0 * 32 * 2 * 56 * 56
    assert eng._wg_cum == 2 * cost and eng._wg_deferred == []
    # both marks were looked at after the launch (3 library calls made), each with its site already registered
    assert eng.marks == [(3, 1, cost), (3, 2, 2 * cost)]
    assert (eng.launches, eng.like_heads) == (1, 2)


def test_declined_paths_issue_nothing_and_leave_the_tape_alone():
    from causal_gen_amd import engine as E

    good = lambda: (_site("x_loc", 3, 0xA000), _site("x_logscale", 4, 0xB000))
    cases = {
        "CGEN_LIKE_HEAD=0": (dict(knob=False), good(), 0),
        "an inference pass": (dict(recording=False), good(), 0),
        "the f32 engine": (dict(dt=E.F32), good(), 0),
        "per-site timing": (dict(prof={}), good(), 0),
        "a frozen logscale weight": ({}, (_site("x_loc", 3, 0xA000), _site("x_logscale", 4, 0xB000, train_w=False)), 0),
        "a head without bias": ({}, (_site("x_loc", 3, 0xA000, bias=False), _site("x_logscale", 4, 0xB000)), 0),
        "a 3x3 head": ({}, (_site("x_loc", 3, 0xA000, ks=3), _site("x_logscale", 4, 0xB000)), 0),
        "the library declines the shape": ({}, good(), 1),
    }
    for label, (kw, (loc, ls), asked) in cases.items():
        lib = StubLib(served=0)
        eng = _engine(lib, **kw)
        h, x = _tensors(eng)
        mark = eng._next[0]
        assert eng.like_head_fwd(loc, ls, h, x, 8) is None, label
        assert [c[0] for c in lib.calls] == ["dgauss_head_supported"] * asked, label
        assert eng.tape == [] and eng._next[0] == mark and eng.like_heads == 0, label  # nothing recorded, nothing allocated


def test_rgb_pixels_are_declined_before_the_library_is_asked():
    lib = StubLib()
    eng = _engine(lib)
    h, _ = _tensors(eng)
    x3 = eng.new(2, 56, 56, 3, rg=False)
    assert eng.like_head_fwd(_site("x_loc", 3, 0xA000), _site("x_logscale", 4, 0xB000), h, x3, 8) is None
    assert lib.calls == []
