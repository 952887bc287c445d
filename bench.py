#!/usr/bin/env python3
"""Benchmark of the HVAE train step (and the counterfactual loop) on MI355X.

    python bench.py --gpus N --steps K --warmup W            # N=1 directly, N>1 under torch.distributed.run
    python bench.py ... --full                               # + everything beyond the headline (see below)
    python bench.py ... --dump-outputs DIR                   # + what the last timed step computed, as DIR/*.npy

A "step" is one pass of the hot path over one synthetic batch already resident in HBM: weight images -> HVAE forward
-> hand-written backward -> (DP: RCCL gradient all-reduce) -> grad-norm / clip / skip -> fused AdamW + EMA.
Prints ONE JSON line on rank 0 (contract in the task description).  A plain run sets up, warms up, times the K steps and
prints the headline (images/s, ms_per_step).  With --full the same line also carries the `roofline` of the dominant
kernel class (measured live with HIP events on the launch stream over one profiled step of the same workload),
`launches_per_step`, the counterfactual loop, the f32 parity leg, the other configs, the batch sweep, the bandwidth
kernels and the `cpu_baseline` (the oracle = bit-matched restatement of the reference's PyTorch-CPU path, timed on this
host); --no-cpu / --no-cf / --no-f32 / --no-extra drop parts of that.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

# conv FLOPs per trained image (fwd + dgrad + wgrad = 3x forward), SURVEY 8(d) / BASELINE.md section 3
TRAIN_GFLOP_PER_IMG = {"morphomnist": 0.260, "cmnist": 0.275, "ukbb192": 69.19, "mimic192": 27.38, "mimic224": 37.38}
CF_GFLOP = {"morphomnist": 0.185, "cmnist": 0.192, "ukbb192": 47.67, "mimic192": 19.57, "mimic224": 26.71}  # abduct + 2 replays
# what the default counterfactual loop EXECUTES (CGEN_CF_REUSE=1): abduction pass (encoder + posterior decoder pass) + ONE
# prior-only replay; the reconstruction is read off the abduction pass (0.086+0.049 / 0.091+0.050 /
# 23.06+12.31 / 9.12+5.22 / 12.45+7.13 GFLOP)
CF_GFLOP_REUSE = {"morphomnist": 0.135, "cmnist": 0.141, "ukbb192": 35.37, "mimic192": 14.34, "mimic224": 19.58}
MFMA_PEAK_TF = {"f32": 157.3, "f16": 2500.0}  # dense, MI355X_MICROARCH.md
DUMP_SAMPLE = 1 << 22  # parameters per --dump-outputs array (16 MB of float32); larger models are sampled


def synth_batch(name, hp, B, device, seed):
    g = torch.Generator().manual_seed(seed)
    R, C = hp.input_res, hp.input_channels
    x = (torch.randint(0, 256, (B, C, R, R), generator=g).float() - 127.5) / 127.5
    if name == "morphomnist":
        pa = torch.cat([torch.rand(B, 2, generator=g) * 2 - 1,
                        torch.nn.functional.one_hot(torch.randint(0, 10, (B,), generator=g), 10).float()], 1)
    elif name == "cmnist":
        pa = torch.cat([torch.nn.functional.one_hot(torch.randint(0, 10, (B,), generator=g), 10).float() for _ in range(2)], 1)
    elif name == "ukbb192":
        pa = torch.stack([torch.randint(0, 2, (B,), generator=g).float(), torch.randn(B, generator=g),
                          torch.randn(B, generator=g), torch.randint(0, 2, (B,), generator=g).float()], 1)
    else:
        pa = torch.randn(B, hp.context_dim, generator=g)
    # the reference's [B,ctx,R,R] parents (trainer.py:16-21) as the stride-0 view the product's own preprocess_batch hands
    # over; CGEN_BENCH_PA=repeat materialises them (the general, spatially varying path) for an A/B
    pa = pa.to(device)[..., None, None].expand(-1, -1, R, R)
    if os.environ.get("CGEN_BENCH_PA") == "repeat":
        pa = pa.contiguous()
    return x.to(device), pa


def build_model(name, dtype, dmol=False):
    from causal_gen_amd import vae
    from causal_gen_amd.hps import setup_hparams

    hp = setup_hparams(name)
    torch.manual_seed(7)
    m = vae.HVAE(hp)
    if dmol:
        from causal_gen_amd.dmol import DmolNet

        m.likelihood = DmolNet(hp)

    def init_bias(mod):  # main.py:51-55
        if type(mod) == torch.nn.Conv2d:
            torch.nn.init.zeros_(mod.bias)

    m.apply(init_bias)
    m.compute_dtype = dtype
    return m, hp


def cpu_worker(name, nthreads, budget_s):
    """(child process) the oracle's train step at a fixed torch thread count; prints one JSON line."""
    from oracle import hparams as ohp
    from oracle import hvae_ref, train_ref

    torch.set_num_threads(nthreads)
    hp = ohp.make_hparams(name)
    B = 32 if hp.input_res <= 64 else 4
    torch.manual_seed(7)
    sd = hvae_ref.init_state_dict(hp)
    tr = train_ref.RefTrainer(sd, hp)
    g = torch.Generator().manual_seed(1)
    x = (torch.randint(0, 256, (B, hp.input_channels, hp.input_res, hp.input_res), generator=g).float() - 127.5) / 127.5
    pa = torch.randn(B, hp.context_dim, generator=g)[..., None, None].repeat(1, 1, hp.input_res, hp.input_res)
    tr.step(x, pa)  # warm-up
    t0, it = time.time(), 0
    while it < 2 or (time.time() - t0 < budget_s and it < 50):
        tr.step(x, pa)
        it += 1
    print(json.dumps(dict(images_s=B * it / (time.time() - t0), steps=it, batch=B, threads=torch.get_num_threads())), flush=True)


def cpu_baseline(name, budget_s=8.0, hard_limit_s=75.0):
    """The oracle's train step (fwd + bwd + clip + AdamW + EMA, trainer.py:54-87) on this host's cores, timed at 8, 32 and
    all hardware threads -- each in its own child process (fresh OpenMP pool, hard time limit; torch oversubscribes the
    mkldnn convs on a 128-thread host: round 1's all-threads figure was 4.7x SLOWER than the reference on 8 threads).
    The best of the three is reported with its thread count."""
    import subprocess

    ncpu = os.cpu_count() or 8
    tried, best = {}, None
    for nt in sorted({min(8, ncpu), min(32, ncpu)}):  # (all hardware threads: slower than 8 by 10-20x on these hosts, and past its time limit at 256)
        env = dict(os.environ, OMP_NUM_THREADS=str(nt), MKL_NUM_THREADS=str(nt), HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-worker", name, str(nt), str(budget_s)], env=env,
                               capture_output=True, text=True, timeout=hard_limit_s, cwd=ROOT)
            row = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        except Exception as e:  # timeout / crash at this thread count: recorded, not fatal
            tried[str(nt)] = None
            continue
        tried[str(nt)] = round(row["images_s"], 4)
        if best is None or row["images_s"] > best[0]:
            best = (row["images_s"], nt, row["steps"], row["batch"])
    if best is None:
        return dict(value=None, unit="images/s", cores=None, kind="port", images_s_by_threads=tried, host_threads=ncpu,
                    sample="every thread count exceeded its %.0f s limit" % hard_limit_s)
    return dict(value=best[0], unit="images/s", cores=best[1], kind="port", images_s_by_threads=tried, host_threads=ncpu,
                sample=f"{best[2]} train steps of {name} at batch {best[3]} (fwd+bwd+clip+AdamW+EMA), f32, after 1 warm-up step, "
                       f"best of {sorted(int(k) for k in tried)} torch threads (one child process each)")


def dump_outputs(path, out, model, ema_model):
    """--dump-outputs: what the caller of the timed step holds after the last timed step, as float32 .npy files --
    `elbo_nll_kl` (the step's return value), `params` and `ema_params` (the trained and the EMA weights, concatenated in
    parameters() order).  Above DUMP_SAMPLE weights both weight arrays hold the same fixed, seeded, sorted sample."""
    import numpy as np

    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "elbo_nll_kl.npy"), out.detach().float().cpu().numpy())
    idx = None
    for name, mod in (("params", model), ("ema_params", ema_model)):
        if mod is None:
            continue
        flat = torch.cat([p.detach().reshape(-1).float() for p in mod.parameters()])
        if idx is None and flat.numel() > DUMP_SAMPLE:
            idx = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(0))[:DUMP_SAMPLE].sort().values
        np.save(os.path.join(path, name + ".npy"), (flat if idx is None else flat[idx.to(flat.device)]).cpu().numpy())


def _code_tree_sha():
    """Content hash of the running package sources (tools/tree_sha.py): what the profile summaries are stamped with."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from tree_sha import tree_sha
    return tree_sha(ROOT)


def _stamp(src):
    """{code_tree_sha of the profiled code, code_tree_sha now, stale}: a summary under profiles/ describes THIS code only when the
    two hashes agree (the round-3 line quoted counters of an older commit without saying so)."""
    prof, now = src.get("code_tree_sha"), _code_tree_sha()
    return dict(profiled_code_tree_sha=prof, running_code_tree_sha=now, stale=(prof != now), profiled_git_sha=src.get("code_git_sha"))


def pmc_traffic(kernel_class, dtype):
    """HBM bytes per launch of the dominant kernel class from the committed rocprofv3 PMC passes (FETCH_SIZE and
    WRITE_SIZE collected in separate passes; tools/pmc_traffic.py applies the gfx950 FETCH_SIZE x2 correction).  PMC
    counters cannot be read from inside this process, so this is the figure of the profiled run of the same command; the
    file it came from and the commit that file was last touched in are returned beside it."""
    import glob
    import subprocess

    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_hbm_traffic_{dtype}_b32.json")))
    if not cands:
        return None, None
    path = cands[-1]
    try:
        blob = json.load(open(path))
        val = blob[kernel_class]["hbm_bytes_per_dispatch"]
    except Exception:
        return None, None
    src = blob.get("_source") or {}
    return val, dict(file=os.path.relpath(path, ROOT), method="rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes), FETCH x2 (gfx950)",
                     **_stamp(src))


def pmc_mfma_busy(kernel_class):
    """SQ counters of the dominant kernel class from the committed PMC passes (tools/pmc_insts.sh + tools/pmc_classes.py):
    MFMA-pipe busy share of a wave's lifetime (SQ_VALU_MFMA_BUSY_CYCLES / 4 SQ_WAVE_CYCLES) and VALU / SALU / LDS instructions
    per MFMA -- what north_star calls the MFMA-utilisation counters."""
    import glob

    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_mfma_busy_by_class.json")))
    if not cands:
        return None
    try:
        blob = json.load(open(cands[-1]))
        d = dict(blob[kernel_class])
        d["source"] = dict(file=os.path.relpath(cands[-1], ROOT), **_stamp(blob.get("_source") or {}))
        return d
    except Exception:
        return None


def profile_step(ts, x, pa, dtype, workload_key=None):
    """One eager step with HIP events around every conv launch (on the launch stream) -> per-class totals."""
    eng = ts.eng
    eng.prof = {}
    launches0 = eng.launches
    # Park the stream behind a spin kernel while the host enqueues the whole eager step: otherwise the host (one ctypes call
    # per launch) is slower than the GPU and every event pair would also time the idle gap before its kernel is enqueued.
    torch.cuda.synchronize()
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(int(0.4 * 2.4e9))
    ts._eager(x, pa, ts.beta)
    torch.cuda.synchronize()
    launches_per_step = eng.launches - launches0
    classes = {}
    shapes = {}
    for (kind, ks, ci, co, res), (flops, evs, n) in eng.prof.items():
        ms = sum(a.elapsed_time(b) for a, b in evs)
        c = classes.setdefault(kind, [0.0, 0.0, 0])
        c[0] += flops; c[1] += ms; c[2] += n
        shapes[(kind, ks, ci, co, res)] = (flops, ms, n)
    eng.prof = None
    # fwd and dgrad are the same kernels (conv_tile / conv_ws / conv_kernel): one class for the roofline
    merged = {"conv_fwd+dgrad": [0.0, 0.0, 0], "conv_wgrad": [0.0, 0.0, 0]}
    for k, v in classes.items():  # (fused Block launches "conv_fwd_blk" / "conv_dgrad_blk" are fwd / dgrad work)
        m = merged["conv_wgrad" if k == "conv_wgrad" else "conv_fwd+dgrad"]
        m[0] += v[0]; m[1] += v[1]; m[2] += v[2]
    classes.update(merged)
    dom = max(merged, key=lambda k: merged[k][1])
    flops, ms, n = merged[dom]
    top = sorted(shapes.items(), key=lambda kv: -kv[1][1])
    dump = os.environ.get("CGEN_SHAPE_DUMP")
    if dump and dtype != "f16":
        dump = dump + "." + dtype
    if dump:
        with open(dump, "w") as f:
            for k, v in top:
                f.write("%-10s ks%d ci%-4d co%-4d res%-4d n%-3d ms %8.3f  TF/s %8.2f\n" % (k[0], k[1], k[2], k[3], k[4], v[2], v[1], v[0] / (v[1] * 1e-3) / 1e12))
    top = top[:8]
    traffic, traffic_src = pmc_traffic(dom, dtype) if workload_key == ("ukbb192", 32) else (None, None)
    busy = pmc_mfma_busy(dom) if workload_key == ("ukbb192", 32) and dtype == "f16" else None
    # the same class against the HBM roofline: counter bytes per launch over the live average launch time (this class mixes
    # HBM-bound launches -- the C/4 -> C convs at >= 96x96 run at 4.6 TB/s -- with latency-bound ones)
    hbm = None
    if traffic:
        tbs = traffic / (1e-3 * ms / n) / 1e12
        hbm = dict(achieved_TB_s=tbs, frac_of_8_TB_s=tbs / 8.0, frac_of_6p3_TB_s_achievable=tbs / 6.3)
    return dict(hbm=hbm, 
        bound="mfma", kernel=dom, achieved=flops / (ms * 1e-3) / 1e12, peak=MFMA_PEAK_TF[dtype], unit="TFLOP/s",
        frac=flops / (ms * 1e-3) / 1e12 / MFMA_PEAK_TF[dtype], traffic=traffic, traffic_source=traffic_src, mfma_counters=busy, launches=n, avg_launch_us=1e3 * ms / n,
        algorithmic_flops_per_launch=flops / n, launches_per_step=launches_per_step,
        classes={k: dict(tflops=v[0] / (v[1] * 1e-3) / 1e12 if v[1] else 0.0, ms=v[1], launches=v[2]) for k, v in classes.items()},
        top_shapes=[dict(kind=k[0], ks=k[1], ci=k[2], co=k[3], res=k[4], ms=v[1], tflops=v[0] / (v[1] * 1e-3) / 1e12, n=v[2])
                    for k, v in top])


def cf_parents(pa):
    """train_cf.py:149 feeds a permutation of the batch's parents as `do`."""
    return pa[:, :, 0, 0].roll(1, 0)[..., None, None].expand_as(pa) if pa.stride(2) == 0 else pa.roll(1, 0)


def cf_leg(model, x, pa, config, n_cf=10):
    """Counterfactuals/s of `model` (abduct -> act -> predict as one hipGraph replay per batch) and the FLOPs it executes."""
    from causal_gen_amd.dscm import GraphedCounterfactual

    cfp = cf_parents(pa)
    counterfactual = GraphedCounterfactual(model)
    for _ in range(3):
        counterfactual(x, pa, cfp)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(n_cf):
        counterfactual(x, pa, cfp)
    torch.cuda.synchronize()
    cf_s = x.shape[0] * n_cf / (time.perf_counter() - t1)
    reuse = os.environ.get("CGEN_CF_REUSE", "1") != "0"
    cf_gf = (CF_GFLOP_REUSE if reuse else CF_GFLOP)[config]
    return {"counterfactuals_per_s": cf_s, "cf_tflops": cf_s * cf_gf * 1e9 / 1e12,  # FLOPs the loop executes, not the three-pass figure
            "cf_gflop_per_counterfactual": {"executed": cf_gf, "reference_three_pass": CF_GFLOP[config],
                                            "reconstruction_from_abduction_pass": reuse}}


def cf_path_name(model):
    """What the compliant counterfactual loop computes with (engine.split_mode: f32 storage with hi + lo binary16 MFMA operands)."""
    eng = model.engine()
    return "f32 storage, " + ("3 x f16 split-operand MFMA (hi*hi + hi*lo + lo*hi), f32 accumulate" if getattr(eng, "f32_split", 0) else "f32 MFMA")


def cf_deviation(m_a, m_b, x, pa):
    """max |cf_x| difference between two models holding the SAME weights (f16 path vs f32 parity path) on the benched batch,
    same Philox state: what the reduced precision does to counterfactual pixels (north_star: 1e-3 abs vs the reference)."""
    from causal_gen_amd.dscm import counterfactual

    outs = []
    for mod in (m_a, m_b):
        was = mod.training
        mod.eval()
        eng = mod.engine()
        eng.rng_ptr()
        eng.rng.copy_(torch.tensor([20240608, 0], dtype=torch.int64))
        with torch.no_grad():
            o = counterfactual(mod, x, pa, cf_parents(pa))
        outs.append((o["x"] if isinstance(o, dict) else o).float().clone())
        mod.train(was)
    return float((outs[0] - outs[1]).abs().max())


def f32_leg(a, hp, B, dev, x, pa, m_f16):
    """The PARITY path (exact f32 MFMA chains: the one the 1e-4 ELBO tests hold on) timed in the same run on the same
    workload, with its own roofline (157.3 TF dense f32 MFMA), and the f16 path's ELBO deviation from it on the benched
    batch at identical weights and identical Philox noise."""
    from causal_gen_amd.train import TrainStep

    m32, _ = build_model(a.config, "f32", a.dmol)
    m32 = m32.to(dev)
    ts32 = TrainStep(m32, hp, ema=False, use_graph=not a.no_graph)
    steps = max(5, a.steps // 2)
    for _ in range(3):
        ts32.step(x, pa)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ts32.step(x, pa)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    roof = profile_step(ts32, x, pa, "f32", (a.config, B))  # (traffic: profiles/r*_hbm_traffic_f32_b32.json, stamped like the f16 one)
    # same weights, same noise: the f16-trained parameters go into the f32 model; both draw from one Philox state
    m32.load_state_dict(m_f16.state_dict())
    vals = {}
    for name, mod in (("f16", m_f16), ("f32", m32)):
        was = mod.training
        mod.eval()
        eng = mod.engine()
        eng.rng_ptr()
        eng.rng.copy_(torch.tensor([20240607, 0], dtype=torch.int64))
        with torch.no_grad():
            o = mod(x, pa, beta=hp.beta)
        vals[name] = [float(o[k]) for k in ("elbo", "nll", "kl")]
        mod.train(was)
    rel = [abs(b - f) / max(abs(f), 1e-12) for b, f in zip(vals["f16"], vals["f32"])]
    # ... and of the numeric path that is TIMED: train mode, a recording forward (plain 16-bit trunk -- the remainder planes are an
    # inference feature --, the fused Block kernels, the tape) against the f32 path run the same way, same weights, same noise
    tvals = {}
    for name, mod in (("f16", m_f16), ("f32", m32)):
        was = mod.training
        mod.train()
        if mod.cond_prior:
            mod.decoder.__dict__["drop_cond"] = lambda: (1, 1)  # (one conditioning-dropout outcome for both)
        eng = mod.engine()
        eng.rng_ptr()
        eng.rng.copy_(torch.tensor([20240607, 0], dtype=torch.int64))
        o = mod(x, pa, beta=hp.beta)
        tvals[name] = [float(o[k].detach()) for k in ("elbo", "nll", "kl")]
        mod.decoder.__dict__.pop("drop_cond", None)
        mod.train(was)
    trel = [abs(b - f) / max(abs(f), 1e-12) for b, f in zip(tvals["f16"], tvals["f32"])]
    gf = TRAIN_GFLOP_PER_IMG[a.config]
    img_s = B * steps / dt
    cf32 = cf_leg(m32, x, pa, a.config, n_cf=4) if not a.no_cf else {}
    cfdev = cf_deviation(m_f16, m32, x, pa) if not a.no_cf else None
    cfdev_plain = None
    if not a.no_cf and m_f16.engine().trunk_mode == 1:
        m_f16.engine().trunk_mode = 0
        cfdev_plain = cf_deviation(m_f16, m32, x, pa)
        m_f16.engine().trunk_mode = 1
    del ts32, m32
    torch.cuda.empty_cache()
    return {"images_s": img_s, "counterfactuals_per_s": cf32.get("counterfactuals_per_s"), "cf_tflops": cf32.get("cf_tflops"),
            "f16_vs_f32_cf_maxabs": cfdev, "f16_plain_trunk_vs_f32_cf_maxabs": cfdev_plain, "ms_per_step": 1e3 * dt / steps, "steps": steps, "model_tflops": img_s * gf / 1e3,
            "model_mfma_frac": img_s * gf / 1e3 / MFMA_PEAK_TF["f32"],
            "roofline": {k: roof.get(k) for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "launches", "avg_launch_us", "classes")},
            "elbo_nll_kl_f32": vals["f32"], "elbo_nll_kl_f16": vals["f16"], "f16_vs_f32_elbo_rel": rel[0],
            "f16_vs_f32_nll_rel": rel[1], "f16_vs_f32_kl_rel": rel[2],
            "timed_path": {"what": "train mode, recording forward: plain 16-bit trunk + fused Block kernels, as TrainStep runs it",
                           "elbo_nll_kl_f32": tvals["f32"], "elbo_nll_kl_f16": tvals["f16"], "f16_vs_f32_elbo_rel": trel[0],
                           "f16_vs_f32_nll_rel": trel[1], "f16_vs_f32_kl_rel": trel[2]}}


def side_config(name, dmol, B, dev, steps=10, prep=12, cf=True, parity=True):
    """One more workload in the same run (f16 train step under a hipGraph, synthetic batch resident in HBM): images/s, fraction
    of the dense f16 MFMA peak, counterfactuals/s, and the f16 path's ELBO deviation from the f32 parity path at identical
    weights and noise."""
    from causal_gen_amd.train import TrainStep

    m, hp = build_model(name, "f16", dmol)
    m = m.to(dev)
    ts = TrainStep(m, hp, ema=cf, use_graph=True)
    x, pa = synth_batch(name, hp, B, dev, seed=100)
    out = None
    for _ in range(prep):
        out = ts.step(x, pa)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = ts.step(x, pa)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    img_s = B * steps / dt
    gf = TRAIN_GFLOP_PER_IMG[name]
    r = {"workload": f"{name} HVAE train step ({hp.input_res}x{hp.input_res}x{hp.input_channels}, {'DMoL' if dmol else 'DGauss'} likelihood)",
         "per_gpu_batch": B, "images_s": img_s, "ms_per_step": 1e3 * dt / steps, "steps": steps, "model_tflops": img_s * gf / 1e3,
         "model_mfma_frac": img_s * gf / 1e3 / MFMA_PEAK_TF["f16"], "elbo_nats_per_dim": float(out[0]),
         "launches_per_step_eager": None}
    if cf:
        f16cf = cf_leg(ts.ema_model, x, pa, name, n_cf=6)
        r["f16_loop"] = {"counterfactuals_per_s": f16cf["counterfactuals_per_s"], "cf_tflops": f16cf["cf_tflops"]}
    if parity:
        m32, _ = build_model(name, "f32", dmol)
        m32 = m32.to(dev)
        m32.load_state_dict(m.state_dict())
        if cf:
            # the rate that meets north_star's 1e-3 on the reference-made fixtures: the f32-storage loop (tests/test_gpu_fullsize.py)
            m32e, _ = build_model(name, "f32", dmol)
            m32e = m32e.to(dev)
            m32e.load_state_dict(ts.ema_model.state_dict())
            c32 = cf_leg(m32e, x, pa, name, n_cf=4)
            r["counterfactuals_per_s"], r["cf_tflops"] = c32["counterfactuals_per_s"], c32["cf_tflops"]
            r["cf_path"] = cf_path_name(m32e)
            del m32e
        vals = {}
        for tag, mod in (("f16", m), ("f32", m32)):
            was = mod.training
            mod.eval()
            eng = mod.engine()
            eng.rng_ptr()
            eng.rng.copy_(torch.tensor([20240607, 0], dtype=torch.int64))
            with torch.no_grad():
                o = mod(x, pa, beta=hp.beta)
            vals[tag] = float(o["elbo"])
            mod.train(was)
        r["elbo_f32_same_weights"] = vals["f32"]
        r["f16_vs_f32_elbo_rel"] = abs(vals["f16"] - vals["f32"]) / max(abs(vals["f32"]), 1e-12)
        if cf:
            r["f16_loop"]["vs_f32_cf_maxabs"] = cf_deviation(m, m32, x, pa)
        del m32
    del ts, m
    torch.cuda.empty_cache()
    return r


def bandwidth_kernels(dev):
    """The HBM-bound kernels of the step against the HBM roofline ("report all three"): algorithmic bytes / HIP-event
    time of the stand-alone launch at the ukbb192 shapes (batch 32, f16), next to 6.3 TB/s achievable and 8 TB/s spec."""
    from causal_gen_amd import _lib
    from causal_gen_amd.engine import Engine

    eng = Engine(dev, "f16")
    eng.begin()
    lib = eng.lib
    out = {}

    def timed(fn, nbytes, reps=20):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = 1e3 * e0.elapsed_time(e1) / reps
        gbs = nbytes / us / 1e3
        return {"us": us, "algorithmic_bytes": nbytes, "GB_s": gbs, "frac_of_6.3TBs": gbs / 6300.0, "frac_of_8TBs": gbs / 8000.0}

    B, R, Z = 32, 96, 16
    heads = [eng.new(B, R, R, 2 * Z + 64), eng.new(B, R, R, 2 * Z)]  # prior Block output [p_loc | p_ls | p_feat], posterior [q_loc | q_ls]
    for t in heads:
        eng.fill(t, 0.1)
    p, q = heads
    z = eng.new(B, R, R, Z)
    kl = torch.zeros(B * lib.reparam_kl_chunks(R, R, Z), device=dev)
    n = B * R * R * Z
    eng.rng_ptr()
    out["reparam_kl_fwd_96"] = timed(lambda: lib.reparam_kl_fwd(eng.dt, B, R, R, Z, q.chan(0, Z).cv(), q.chan(Z, 2 * Z).cv(), p.chan(0, Z).cv(),
                                                                  p.chan(Z, 2 * Z).cv(), _lib.NULL_VIEW, eng.rng_ptr(), 7, 0.0, z.cv(), _lib.NULL_VIEW,
                                                                  kl.data_ptr(), kl.numel() // B, eng.stream), n * 2 * 5)  # 4 reads + 1 write
    gq, gp, gz = eng.new(B, R, R, 2 * Z), eng.new(B, R, R, 2 * Z + 64), eng.new(B, R, R, Z)
    eng.fill(gz, 0.01)
    coef = torch.ones(1, device=dev)
    out["reparam_kl_bwd_96"] = timed(lambda: lib.reparam_kl_bwd(eng.dt, B, R, R, Z, q.chan(0, Z).cv(), q.chan(Z, 2 * Z).cv(), p.chan(0, Z).cv(),
                                                                  p.chan(Z, 2 * Z).cv(), z.cv(), 0.0, gz.cv(), coef.data_ptr(), 0, None,
                                                                  gq.chan(0, Z).cv(), gq.chan(Z, 2 * Z).cv(), gp.chan(0, Z).cv(), gp.chan(Z, 2 * Z).cv(), 0, 0,
                                                                  eng.stream), n * 2 * 10)  # 6 reads + 4 writes
    Rx = 192
    params, xin = eng.new(B, Rx, Rx, 2), eng.new(B, Rx, Rx, 1)
    eng.fill(params, 0.0)
    eng.fill(xin, 0.3)
    part = torch.zeros(B * lib.like_chunks(Rx, Rx), device=dev)
    out["dgauss_nll_fwd_192"] = timed(lambda: lib.dgauss_nll_fwd(eng.dt, B, Rx, Rx, 1, params.cv(), xin.cv(), part.data_ptr(), eng.stream),
                                      B * Rx * Rx * 2 * 3)
    gpar = eng.new(B, Rx, Rx, 2)
    out["dgauss_nll_bwd_192"] = timed(lambda: lib.dgauss_nll_bwd(eng.dt, B, Rx, Rx, 1, params.cv(), xin.cv(), coef.data_ptr(), 0, gpar.cv(), eng.stream),
                                      B * Rx * Rx * 2 * 5)
    return out


def main():
    if len(sys.argv) >= 5 and sys.argv[1] == "--cpu-worker":
        return cpu_worker(sys.argv[2], int(sys.argv[3]), float(sys.argv[4]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="ukbb192", choices=sorted(TRAIN_GFLOP_PER_IMG))
    ap.add_argument("--batch", type=int, default=None, help="per-GPU batch (default: 32 at 192^2/224^2, 256 at 32^2)")
    ap.add_argument("--dtype", default="f16", choices=["f32", "f16"])
    ap.add_argument("--dmol", action="store_true", help="DMoL likelihood head (cmnist)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--full", action="store_true", help="after the headline also measure the roofline, the counterfactual loop, the f32 parity "
                                                         "leg, the other configs, the batch sweep, the bandwidth kernels and the CPU baseline")
    ap.add_argument("--no-cpu", action="store_true", help="(--full) skip the CPU baseline")
    ap.add_argument("--no-cf", action="store_true", help="(--full) skip the counterfactual loop")
    ap.add_argument("--no-f32", action="store_true", help="(--full) skip the f32 parity-path leg (timed after the f16 headline at N=1)")
    ap.add_argument("--no-extra", action="store_true", help="(--full) skip the other BASELINE configs, the batch sweep and the bandwidth-kernel table (default ukbb192 run only)")
    ap.add_argument("--prep-steps", type=int, default=20, help="untimed optimiser steps so the prior heads are non-zero")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one computed (ELBO / NLL / KL, trained and EMA weights) as DIR/*.npy")
    a = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: start one rank per GPU ourselves (the driver's torch.distributed.run form sets
        # WORLD_SIZE and lands below).  With fewer devices than ranks the ranks share them (local % device_count): a dry run of
        # the DP path, which RCCL refuses (two ranks on one device) -- say CGEN_DIST_BACKEND=gloo for that.
        import socket
        import subprocess

        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))))
    if world != a.gpus:
        sys.exit(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world} (launched under torch.distributed.run with a different --nproc-per-node)")
    local = local % max(torch.cuda.device_count(), 1)  # (a 1-GPU box can host a 2-rank gloo dry run of the DP path)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    pg = None
    # more than one rank -- or a ONE-rank dry run of the same code through RCCL (CGEN_DP_FORCE=1 under torch.distributed.run):
    # process group, barriers, max-over-ranks timing, split backward graph and bucketed all-reduces, on a single GPU
    distributed = world > 1 or (os.environ.get("CGEN_DP_FORCE") == "1" and "WORLD_SIZE" in os.environ)
    if distributed:
        import torch.distributed as dist

        backend = os.environ.get("CGEN_DIST_BACKEND", "nccl")  # nccl == RCCL on ROCm
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
        pg = dist.group.WORLD
        seen = torch.ones(1, device=dev)
        dist.all_reduce(seen)  # every rank adds 1 through the collective the gradients use: the ranks that backend really reached
        ranks_seen = int(seen.item())

    from causal_gen_amd.train import TrainStep

    m, hp = build_model(a.config, a.dtype, a.dmol)
    m = m.to(dev)
    B = a.batch or (256 if hp.input_res <= 64 else 32)
    ts = TrainStep(m, hp, ema=True, use_graph=not a.no_graph, process_group=pg)
    x, pa = synth_batch(a.config, hp, B, dev, seed=100 + rank)

    out = None
    for _ in range(a.prep_steps + a.warmup):
        out = ts.step(x, pa)

    def sync():
        if distributed:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    sync()
    ts.time_comm = distributed
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = ts.step(x, pa)
    sync()
    dt = time.perf_counter() - t0
    ts.time_comm = False
    exposed_comm = ts.exposed_comm_ms() if distributed else None
    if distributed:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t.item())
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, out, m, ts.ema_model)  # (before anything below steps the model again)
    elbo, nll, kl = [float(v) for v in out.cpu()]
    stats = ts.stats()
    img_s = B * world * a.steps / dt
    # the profiled eager step contains the gradient all-reduce: every rank takes part (rank 0 reports)
    roof = profile_step(ts, x, pa, a.dtype, (a.config, B)) if a.full else None

    if rank == 0:
        gf = TRAIN_GFLOP_PER_IMG[a.config]
        res = {
            "metric": "HVAE train images/sec", "value": img_s, "unit": "images/s", "n_gpus": world, "steps": a.steps,
            "warmup": a.warmup, "ms_per_step": 1e3 * dt / a.steps, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": a.dtype, "data": "synthetic",
            "config": {"workload": f"{a.config} HVAE train step ({hp.input_res}x{hp.input_res}x{hp.input_channels}, "
                                   f"{'DMoL' if a.dmol else 'DGauss'} likelihood, beta={hp.beta}, z_max_res={hp.z_max_res})",
                       "per_gpu_batch": B, "global_batch": B * world, "parallelism": f"dp{world}",
                       "hipgraph": not a.no_graph, "params": sum(p.numel() for p in m.parameters())},
            "elbo_nats_per_dim": elbo, "nll": nll, "kl": kl, "opt_steps": stats["opt_steps"], "skipped": stats["n_skipped"],
            "wgrad_partial_bytes_per_step": sum(e[0].numel() * 4 for e in ts.eng._partials.values()),
            "arena_bytes": ts.eng.arena.high_water,
            "model_tflops": img_s * gf * 1e9 / 1e12,
            "model_mfma_frac": img_s * gf * 1e9 / 1e12 / (MFMA_PEAK_TF[a.dtype] * world),
            "param_abs_sum": float(sum(p.detach().double().abs().sum() for p in m.parameters())),
        }
        if distributed:
            res["dp"] = {"allreduce_overlapped_with_backward": bool(ts.dp_overlap and ts.early_ranges),
                         "exposed_comm_ms_per_step": exposed_comm,
                         "early_bytes": 4 * sum(hi - lo for lo, hi in (ts.early_ranges or [])),
                         "late_bytes": 4 * sum(hi - lo for lo, hi in (ts.late_ranges or [(0, ts._gbuf().numel())])),
                         # bus bandwidth the exchange actually reached (ring: 2 (N-1)/N x bytes over the time the all-reduce
                         # was exposed); meaningful for the serialized form, where all of it is exposed -- the number the
                         # overlap policy's assumed CGEN_DP_BUS_GBS (300) should be re-decided from
                         "bus_GB_s_achieved": (None if not exposed_comm else
                                               2.0 * (world - 1) / max(world, 1) * 4.0 * ts._gbuf().numel() / (exposed_comm * 1e-3) / 1e9),
                         "gradient_bytes": 4 * ts._gbuf().numel(),
                         "overlap_policy": getattr(ts, "dp_policy", None),
                         "backend": os.environ.get("CGEN_DIST_BACKEND", "nccl"),
                         ("rccl_ranks_seen" if os.environ.get("CGEN_DIST_BACKEND", "nccl") == "nccl" else "gloo_ranks_seen"): ranks_seen,
                         "devices_visible": torch.cuda.device_count()}
        if a.full:
            res["launches_per_step"] = roof.get("launches_per_step")
            res["roofline"] = roof
        if a.full and not a.no_cf:
            # top-level counterfactuals_per_s = the loop that meets north_star's 1e-3 absolute on the reference-made fixtures
            # (tests/test_gpu_fullsize.py): f32 storage (cf_path says which MFMAs).  The all-16-bit loop is reported beside it
            # as `f16_loop`, labelled with the bound it is held to (5e-3) and its deviation on this batch.
            f16cf = cf_leg(ts.ema_model, x, pa, a.config) if a.dtype == "f16" else None
            m32cf, _ = build_model(a.config, "f32", a.dmol)
            m32cf = m32cf.to(dev)
            m32cf.load_state_dict(ts.ema_model.state_dict())
            m32cf.eval()
            res.update(cf_leg(m32cf, x, pa, a.config, n_cf=6))
            res["cf_path"] = cf_path_name(m32cf)
            res["cf_pixel_bound_held_vs_reference"] = 1e-3
            if f16cf is not None:
                res["f16_loop"] = {"counterfactuals_per_s": f16cf["counterfactuals_per_s"], "cf_tflops": f16cf["cf_tflops"],
                                   "pixel_bound_held_vs_reference": 5e-3,
                                   "vs_f32_cf_maxabs_this_batch": cf_deviation(ts.ema_model, m32cf, x, pa)}
            del m32cf
            torch.cuda.empty_cache()
        if a.full and world == 1 and a.dtype == "f16" and not a.no_f32:
            res["f32"] = f32_leg(a, hp, B, dev, x, pa, m)
        if a.full and world == 1 and not a.no_extra and a.config == "ukbb192" and a.batch is None and a.dtype == "f16":
            # the other BASELINE.json configs and a per-GPU batch sweep of the headline model, same process, same code
            del ts
            torch.cuda.empty_cache()
            res["bandwidth_kernels"] = bandwidth_kernels(dev)
            res["configs"] = {}
            for key, cfg, dmol, Bc in (("morphomnist_b256", "morphomnist", False, 256), ("cmnist_dmol_b256", "cmnist", True, 256),
                                       ("mimic224_b32", "mimic224", False, 32)):
                res["configs"][key] = side_config(cfg, dmol, Bc, dev)
            res["batch_sweep_ukbb192"] = {str(Bs): side_config("ukbb192", False, Bs, dev, cf=False, parity=False) for Bs in (64, 128)}
        if "f32" in res:
            f = res["f32"]
            res["parity"] = {
                "north_star": "ELBO / nats-per-dim within 1e-4 relative, counterfactual pixels within 1e-3 absolute of the reference CPU path",
                "f32_path": "held at 1e-4 / 1e-3 against the reference-made full-size fixtures on all four presets (tests/test_gpu_fullsize.py)",
                "f16_timed_path_vs_f32_elbo_rel": f["timed_path"]["f16_vs_f32_elbo_rel"],
                "f16_inference_path_vs_f32_elbo_rel": f["f16_vs_f32_elbo_rel"],
                "counterfactuals": {"per_s": res.get("counterfactuals_per_s"), "path": res.get("cf_path"), "pixel_bound_held_vs_reference": 1e-3,
                                    "f16_loop_per_s": (res.get("f16_loop") or {}).get("counterfactuals_per_s"),
                                    "f16_loop_vs_f32_pixels_maxabs_this_batch": f["f16_vs_f32_cf_maxabs"],
                                    "f16_loop_pixel_bound_held_vs_reference": 5e-3,
                                    "note": "counterfactuals_per_s at top level is the loop that meets north_star's 1e-3 on the reference-made "
                                            "fixtures (f32 storage); f16_loop is the all-16-bit approximation, a 5e-3 number on those fixtures"}}
        if a.full and world == 1 and not a.no_cpu:
            res["cpu_baseline"] = cpu_baseline(a.config)
        print(json.dumps(res))
    if distributed:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
