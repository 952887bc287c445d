"""The decoder layers' backward latent tail in a rocprofv3 kernel trace (csv) of bench.py, per layer size: the launches that run
between a layer's conv-Block backward and its prior / posterior Block backward.  In the four-launch path these are the 1x1 data
gradients (conv_px / conv_smallp / conv_tile kernels) followed by reparam_kl_bwd; in the fused path one latent_tail_bwd_kernel.
Same step selection as tools/timeline.py (the shortest whole step = a graph replay).
The forward tails are reported as well: per layer the reparam_kl_fwd launch and the two 1x1 convs over [z | .] behind it (z_proj on
the reparam's queue, z_feat_proj usually on the side queue) -- first start .. last end of the three, and the main-chain part alone
(reparam start .. z_proj end); in the fused path one latent_tail_fwd_kernel.
Last, the DETERMINISTIC layers at the top resolution (no reparam launch marks them): every launch between the last upsample and the
likelihood head, and between elbo_finalize and the first upsample_bwd, that is neither a Block nor the head -- the 1x1 convs, their
data gradients, the landed rider and the zero fill, or latent_tail_det_fwd_kernel / latent_tail_det_bwd_kernel.
usage: python tools/lat_tail_timeline.py <kernel_trace.csv> [out.txt]"""
import collections
import csv
import sys

import re

rows = []
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"])),
                     int(r["Grid_Size_Y"]), int(r["LDS_Block_Size"]), int(r.get("Queue_Id", 0) or 0)))
rows.sort()
commits = [i for i, r in enumerate(rows) if "step_commit" in r[2]]
step, best = None, None
for a_, b_ in zip(commits[:-1], commits[1:]):
    if b_ - a_ > 300:
        cand = rows[a_ + 1:b_ + 1]
        span = max(r[1] for r in cand) - cand[0][0]
        if step is None or span < best:
            step, best = cand, span
assert step is not None, "no train step in the trace"


def short(n):
    return n.split("(")[0].replace("void ", "").replace("cgen::", "")[:44]


def is_block(n):
    return "blk3" in n or "blk4" in n


out = []
P = out.append
groups = collections.OrderedDict()  # (signature of the tail) -> list of [durations per launch], span
fin = next((k for k, r in enumerate(step) if "elbo_finalize" in r[2]), 0)
k = fin
while k < len(step):
    n = step[k][2]
    if "reparam_kl_bwd" in n or "latent_tail_bwd" in n:
        j, convs = k, 0  # walk back over this layer's (at most three) 1x1 data gradients; a pair launch stands for two of them
        while "reparam" in n and j - 1 > fin and convs < 3 and any(t in step[j - 1][2] for t in ("conv_px", "conv_smallp", "conv_tile")):
            j -= 1
            convs += 2 if "pair" in step[j][2] else 1
        tail = step[j:k + 1]
        nxt = step[k + 1] if k + 1 < len(step) else None  # (the Block backward behind the tail: tells layer sizes with equal tail grids apart)
        sig = tuple((short(r[2]), r[3], r[4]) for r in tail) + ((("then " + short(nxt[2]))[:44], nxt[3], nxt[4]),) * (nxt is not None)
        g = groups.setdefault(sig, [[], []])
        g[0].append([(r[1] - r[0]) / 1e3 for r in tail])
        g[1].append((tail[-1][1] - tail[0][0]) / 1e3)
    k += 1
total = 0.0
P("backward latent tails of the step, grouped by their launches (kernel, workgroups x parts): count, mean us per launch, mean first-start .. last-end us")
for sig, (durs, spans) in groups.items():
    cnt = len(durs)
    mean = [sum(d[c] for d in durs) / cnt for c in range(len(durs[0]))]
    total += sum(spans)
    P("  x%-3d span %6.1f us" % (cnt, sum(spans) / cnt))
    for (name, gx, gy), m in zip(sig, mean + [None]):
        P("        %9s  %-44s %5d x %d" % ("" if m is None else "%6.1f us" % m, name, gx, gy))
P("sum of the tails' spans: %.3f ms in %d layers" % (total / 1e3, sum(len(v[0]) for v in groups.values())))
lastd = None
for r in step:
    if ("conv_" in r[2] or "blk_kernel" in r[2]) and "wgrad" not in r[2]:
        lastd = r
P("step span %.3f ms; backward chain (elbo_finalize end .. last fwd/dgrad conv end) %.3f ms; kernels in the step %d"
  % ((max(r[1] for r in step) - step[0][0]) / 1e6, (lastd[1] - step[fin][1]) / 1e6, len(step)))

# ---- forward tails: everything before elbo_finalize
CAT1X1 = re.compile(r"conv_px_kernel<\d+, 1, false|conv_smallp_kernel<1, \d+, \d+, false|conv_tile_kernel")  # a 1x1 conv over two segments
fgroups = collections.OrderedDict()  # signature -> [durations per launch], spans, main-chain spans
k = 0
while k < fin:
    n = step[k][2]
    if "reparam_kl_fwd" in n or "latent_tail_fwd" in n:
        cand, j = [], k + 1
        while "reparam" in n and j < fin and j <= k + 6 and "reparam_kl_fwd" not in step[j][2]:
            if CAT1X1.search(step[j][2]):
                cand.append(step[j])
            j += 1
        # z_proj is the first such conv on the reparam's queue; z_feat_proj the first one on another (the side) queue, or -- where the
        # next layer has no prior chain to run ahead (the last stochastic layer) -- the second one on the reparam's own, behind the conv Block
        mine, side = [r for r in cand if r[6] == step[k][6]], [r for r in cand if r[6] != step[k][6]]
        tail = sorted([step[k]] + mine[:1] + (side[:1] if side else mine[1:2]))
        same_q = [r for r in tail[1:] if r[6] == tail[0][6]]
        zproj = same_q[0] if same_q else (tail[1] if len(tail) > 1 else tail[0])
        sig = tuple((short(r[2]), r[3], r[4]) for r in tail)
        g = fgroups.setdefault(sig, [[], [], []])
        g[0].append([(r[1] - r[0]) / 1e3 for r in tail])
        g[1].append((max(r[1] for r in tail) - tail[0][0]) / 1e3)
        g[2].append((zproj[1] - tail[0][0]) / 1e3)
    k += 1
P("forward latent tails of the step, grouped by their launches (kernel, workgroups x parts): count, mean us per launch, mean first-start .. last-end us, mean main-chain part (reparam start .. z_proj end) us")
ftotal = fmain = 0.0
for sig, (durs, spans, mains) in fgroups.items():
    cnt = len(durs)
    mean = [sum(d[c] for d in durs) / cnt for c in range(len(durs[0]))]
    ftotal += sum(spans)
    fmain += sum(mains)
    P("  x%-3d span %6.1f us   main chain %6.1f us" % (cnt, sum(spans) / cnt, sum(mains) / cnt))
    for (name, gx, gy), m in zip(sig, mean):
        P("        %9s  %-44s %5d x %d" % ("%6.1f us" % m, name, gx, gy))
P("sum of the forward tails' spans: %.3f ms, of their main-chain parts: %.3f ms, in %d layers; forward chain (step start .. elbo_finalize start) %.3f ms"
  % (ftotal / 1e3, fmain / 1e3, sum(len(v[0]) for v in fgroups.values()), (step[fin][0] - step[0][0]) / 1e6))

# ---- the deterministic layers at the top resolution (z = p_loc: no reparam launch marks them): forward, what runs between the last
# upsample and the likelihood head that is neither a Block nor the head; backward, the same between elbo_finalize and the first
# upsample_bwd.  Separate launches: 1x1 convs over [p_loc | .] / their data gradients, the landed rider (axpby) and the zero fill of
# grad(p_ls); fused: latent_tail_det_fwd_kernel / latent_tail_det_bwd_kernel.
def det_rows(lo, hi):
    skip = ("blk3", "blk4", "dgauss", "elbo_finalize", "upsample", "nll")
    return [r for r in step[lo:hi] if not any(s in r[2] for s in skip)]


ups_f = [k for k in range(fin) if "upsample_fwd" in step[k][2]]
ups_b = [k for k in range(fin, len(step)) if "upsample_bwd" in step[k][2]]
if ups_f and ups_b:
    t0 = step[0][0]
    for title, rows_ in (("forward", det_rows(ups_f[-1] + 1, fin)), ("backward", det_rows(fin + 1, ups_b[0]))):
        P("deterministic top-resolution layers, %s: start us | us | kernel | workgroups x parts" % title)
        for r in rows_:
            P("    %9.1f | %6.1f | %-44s | %5d x %d" % ((r[0] - t0) / 1e3, (r[1] - r[0]) / 1e3, short(r[2]), r[3], r[4]))
        P("  %d launches, sum %.1f us" % (len(rows_), sum(r[1] - r[0] for r in rows_) / 1e3))
txt = "\n".join(out)
print(txt)
if len(sys.argv) > 2:
    open(sys.argv[2], "a").write(txt + "\n")
