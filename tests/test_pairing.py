"""The pair slot of the backward pass (causal_gen_amd/pairing.py) with fake launch functions: exact event sequences and counters.
No GPU, no library."""
from types import SimpleNamespace

import pytest

from causal_gen_amd.pairing import BlockRec, PairSlot, may_pair


def _slot(supported=True, prof=None):
    ev = []
    eng = SimpleNamespace(launches=10, prof=prof)

    def single(a, info):
        assert info == "info-" + a  # (what the single-launch path needs travels with the held launch)
        eng.launches += 1           # (as Engine._timed does)
        ev.append("single(%s)" % a)

    slot = PairSlot(eng, single, lambda h, a: ev.append("pair(%s,%s)" % (h, a)), lambda h, a: supported)
    return slot, eng, ev


def _submit(slot, ev, a, writes, reads):
    slot.submit(a, set(writes), set(reads), "info-" + a, lambda: ev.append("late(%s)" % a))


SPLIT = ["single(A)", "late(A)", "single(B)", "late(B)"]


def test_compatible_launches_share_one():
    slot, eng, ev = _slot()
    slot.arm()
    _submit(slot, ev, "A", {"gA"}, {"x", "tA"})
    assert ev == [] and eng.launches == 10 and slot.held is not None and not slot.armed  # held: nothing launched, no late
    _submit(slot, ev, "B", {"gB"}, {"x", "tB"})  # (both may READ the same tensor)
    assert ev == ["pair(A,B)", "late(A)", "late(B)"]
    assert slot.pairs == 1 and eng.launches == 11 and not slot.busy


@pytest.mark.parametrize("b_writes,b_reads", [
    (("tA",), ("tB",)),   # B writes something A reads
    (("gB",), ("gA",)),   # A writes something B reads
    (("gA",), ("tB",)),   # A writes something B writes
], ids=["b-writes-a-read", "a-writes-b-read", "a-writes-b-write"])
def test_a_hazard_splits_the_pair(b_writes, b_reads):
    slot, eng, ev = _slot()
    slot.arm()
    _submit(slot, ev, "A", {"gA"}, {"tA"})
    _submit(slot, ev, "B", b_writes, b_reads)
    assert ev == SPLIT and slot.pairs == 0 and eng.launches == 12 and not slot.busy


def test_a_launch_between_hold_and_partner_splits_the_pair():
    slot, eng, ev = _slot()
    slot.arm()
    _submit(slot, ev, "A", {"gA"}, {"tA"})
    eng.launches += 1  # (a fill, a residual copy, a background flush ...)
    _submit(slot, ev, "B", {"gB"}, {"tB"})
    assert ev == SPLIT and slot.pairs == 0 and eng.launches == 13 and not slot.busy


def test_an_unsupported_pair_is_split():
    slot, eng, ev = _slot(supported=False)
    slot.arm()
    _submit(slot, ev, "A", {"gA"}, {"tA"})
    _submit(slot, ev, "B", {"gB"}, {"tB"})
    assert ev == SPLIT and slot.pairs == 0 and eng.launches == 12 and not slot.busy


def test_flush_launches_the_held_one_alone_once():
    slot, eng, ev = _slot()
    slot.arm()
    _submit(slot, ev, "A", {"gA"}, {"tA"})
    slot.flush()
    assert ev == ["single(A)", "late(A)"] and eng.launches == 11 and not slot.busy
    slot.flush()
    assert ev == ["single(A)", "late(A)"] and eng.launches == 11 and slot.pairs == 0


def test_flush_disarms():
    slot, eng, ev = _slot()
    slot.arm()
    slot.flush()
    assert ev == [] and not slot.busy


def test_profiling_never_holds():
    slot, eng, ev = _slot(prof={})
    slot.arm()
    _submit(slot, ev, "A", {"gA"}, {"tA"})
    assert ev == ["single(A)", "late(A)"] and slot.held is None and eng.launches == 11 and slot.pairs == 0


def test_disarmed_without_a_submit_the_next_one_goes_out_at_once():
    slot, eng, ev = _slot()
    slot.arm()
    slot.disarm()
    _submit(slot, ev, "A", {"gA"}, {"tA"})
    assert ev == ["single(A)", "late(A)"] and not slot.busy and eng.launches == 11


def test_disarm_leaves_a_held_launch_alone():
    slot, eng, ev = _slot()
    slot.arm()
    _submit(slot, ev, "A", {"gA"}, {"tA"})
    slot.disarm()
    assert ev == [] and slot.held is not None and slot.busy
    _submit(slot, ev, "B", {"gB"}, {"tB"})
    assert ev == ["pair(A,B)", "late(A)", "late(B)"] and slot.pairs == 1


def test_reset_drops_a_held_launch():
    slot, eng, ev = _slot()
    slot.arm()
    _submit(slot, ev, "A", {"gA"}, {"tA"})
    slot.reset()
    assert ev == [] and not slot.busy and slot.held is None and eng.launches == 10
    slot.flush()
    assert ev == []


def test_an_idle_slot_launches_alone():
    slot, eng, ev = _slot()
    assert not slot.busy  # (the conv path does not even consult the slot then)
    _submit(slot, ev, "A", {"gA"}, {"tA"})
    assert ev == ["single(A)", "late(A)"] and not slot.busy and slot.pairs == 0 and eng.launches == 11


def test_late_is_optional():
    slot, eng, ev = _slot()
    slot.arm()
    slot.submit("A", {"gA"}, {"tA"}, "info-A")
    slot.submit("B", {"gB"}, {"tB"}, "info-B")
    assert ev == ["pair(A,B)"] and slot.pairs == 1 and eng.launches == 11


# ---------------------------------------------------------------------------------------------------------- the arming rule
def _t(h=24, w=24, rg=True, base=None):
    t = SimpleNamespace(h=h, w=w, rg=rg)
    t.base = t if base is None else base
    return t


def _entry(fn, segs, out=None, res1=None):
    return (fn, BlockRec(("s1", "s2"), segs, (_t(),), out if out is not None else _t(), res1), 0)


def test_may_pair_posterior_then_prior():
    pa = _t(rg=False)
    post = _entry("bw3", [_t(), pa, _t()])
    prior = _entry("bw3", [_t(), pa])  # (sharing an input that needs no gradient is fine)
    assert may_pair(post, prior)
    fn, args, _ = post
    assert args.sites == ("s1", "s2") and len(tuple(args)) == 5  # (fn(*args) still works)


def test_may_pair_needs_a_next_entry_of_the_same_kind():
    post = _entry("bw3", [_t()])
    assert not may_pair(post, None)
    assert not may_pair(post, _entry("bw4", [_t()]))
    assert may_pair(post, _entry("bw3", [_t()]))


def test_may_pair_refuses_a_residual_partner():
    post = _entry("bw3", [_t()])
    assert not may_pair(post, _entry("bw3", [_t()], res1=_t()))
    assert may_pair(_entry("bw3", [_t()], res1=_t()), _entry("bw3", [_t()]))  # (only the NEXT entry's residual counts)


@pytest.mark.parametrize("h,w,ok", [(24, 24, True), (12, 24, False), (24, 12, False)])
def test_may_pair_needs_the_same_image_size(h, w, ok):
    assert may_pair(_entry("bw3", [_t(24, 24)]), _entry("bw3", [_t(h, w)])) == ok


def test_may_pair_refuses_a_shared_differentiable_input():
    x = _t()
    assert not may_pair(_entry("bw3", [x]), _entry("bw3", [_t(), _t(base=x)]))  # (a channel slice of the same storage)
    frozen = _t(rg=False)
    assert may_pair(_entry("bw3", [_t(), frozen]), _entry("bw3", [_t(), _t(rg=False, base=frozen)]))


def test_may_pair_refuses_a_partner_that_produced_an_input():
    y = _t()
    assert not may_pair(_entry("bw3", [_t(base=y)]), _entry("bw3", [_t()], out=y))
    assert not may_pair(_entry("bw3", [_t(), _t(rg=False, base=y)]), _entry("bw3", [_t()], out=y))  # (differentiable or not)
    assert may_pair(_entry("bw3", [_t()]), _entry("bw3", [_t()], out=y))
