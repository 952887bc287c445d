"""Time the two multi-tensor launches at the step boundary on their own: the weight re-imaging (Engine.prepare_weights) and the split-K
reductions of a real backward pass (WgradMixin._reduce_round), the reductions with the per-element reference kernel and with the tiled one.
Builds the preset's model and engine as bench.py does, runs two eager training steps so that the reduce tables of the step exist, then
replays every launch alone: 3 warm-up, 20 timed, HIP events.  Prints microseconds, the bytes the launch has to move and bytes / time.
For the table in LABNOTES 22; not a test.

    python tools/bench_step_boundary.py [--config ukbb192] [--dmol] [--batch 32]"""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warm=3, reps=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ts = sorted(ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(reps))
    return ts[len(ts) // 2], ts[0], ts[-1]


def row(label, nwork, us, nbytes):
    med, lo, hi = us
    print(f"  {label:<28} {nwork:>7} workgroups  {med:8.1f} us (min {lo:.1f}, max {hi:.1f})  {nbytes / 1e6:8.1f} MB  {nbytes / med / 1e6:6.2f} TB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="ukbb192")
    ap.add_argument("--dmol", action="store_true")
    ap.add_argument("--batch", type=int, default=0)
    a = ap.parse_args()
    import bench
    from causal_gen_amd import _lib
    from causal_gen_amd.train import TrainStep

    dev = torch.device("cuda")
    m, hp = bench.build_model(a.config, "f16", a.dmol)
    m = m.to(dev)
    B = a.batch or (256 if hp.input_res <= 64 else 32)
    ts = TrainStep(m, hp, ema=True, use_graph=False)
    x, pa = bench.synth_batch(a.config, hp, B, dev, seed=100)
    for _ in range(2):
        ts.step(x, pa)
    torch.cuda.synchronize()
    eng = ts.eng
    st = torch.cuda.current_stream(dev).cuda_stream
    lib = eng.lib

    d, cs, ci, n = eng._prep_tab
    raw = bytes(d.cpu().numpy())
    descs = (_lib.WprepDesc * (len(raw) // C.sizeof(_lib.WprepDesc))).from_buffer_copy(raw)
    img_bytes = sum(q.numel * (4 if q.dtype == _lib.F32 and q.mode <= 1 else 2) for q in descs)
    par_bytes = 4 * sum(s.conv.weight.numel() for s in eng.sites)
    by_mode = {}
    for q in descs:
        by_mode[q.mode] = by_mode.get(q.mode, 0) + q.numel * (4 if q.dtype == _lib.F32 and q.mode <= 1 else 2)
    print(f"{a.config}{' + DMoL' if a.dmol else ''}, batch {B}: {len(eng.sites)} conv sites, {par_bytes / 1e6:.1f} MB of conv parameters, "
          f"{len(descs)} images of {img_bytes / 1e6:.1f} MB (buffer {eng._img_buf.numel() / 1e6:.1f} MB)")
    print("  image MB by mode: " + ", ".join(f"{k}: {v / 1e6:.1f}" for k, v in sorted(by_mode.items())))
    print("weight re-imaging (bytes = parameters read once + images written)")
    row("cgen_weight_prep_ref", n, timed(lambda: lib.weight_prep_ref(d.data_ptr(), cs.data_ptr(), ci.data_ptr(), n, st)), par_bytes + img_bytes)

    print("split-K reductions of one backward pass (bytes = partials read + gradient written)")
    for k, tab in enumerate(eng._red_tabs.values()):
        rd, rcs, rci, rn, ritems, rnitems = tab
        raw = bytes(rd.cpu().numpy())
        rdescs = (_lib.WredDesc * (len(raw) // C.sizeof(_lib.WredDesc))).from_buffer_copy(raw)
        nbytes = 4 * sum(q.numel * (q.nsplit + 1 + q.accumulate) for q in rdescs)
        ns = sorted(q.nsplit for q in rdescs)
        deep = sum(q.numel for q in rdescs if q.nsplit > 16)
        print(f"  launch {k}: {len(rdescs)} sites, {sum(q.numel for q in rdescs) / 1e6:.2f} M elements, nsplit min {ns[0]} median {ns[len(ns) // 2]} max {ns[-1]}, "
              f"{deep / 1e3:.0f} k elements behind more than 16 splits, layout 1: {sum(1 for q in rdescs if q.layout == 1)} sites")
        row("cgen_wgrad_reduce_ref", rn, timed(lambda: lib.wgrad_reduce_ref(rd.data_ptr(), rcs.data_ptr(), rci.data_ptr(), rn, st)), nbytes)
        row("cgen_wgrad_reduce_tiles", rnitems, timed(lambda: lib.wgrad_reduce_tiles(ritems.data_ptr(), rnitems, st)), nbytes)


if __name__ == "__main__":
    main()
