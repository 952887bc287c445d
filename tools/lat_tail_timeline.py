"""The decoder layers' backward latent tail in a rocprofv3 kernel trace (csv) of bench.py, per layer size: the launches that run
between a layer's conv-Block backward and its prior / posterior Block backward.  In the four-launch path these are the 1x1 data
gradients (conv_px / conv_smallp / conv_tile kernels) followed by reparam_kl_bwd; in the fused path one latent_tail_bwd_kernel.
Same step selection as tools/timeline.py (the shortest whole step = a graph replay).
usage: python tools/lat_tail_timeline.py <kernel_trace.csv> [out.txt]"""
import collections
import csv
import sys

rows = []
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"])),
                     int(r["Grid_Size_Y"]), int(r["LDS_Block_Size"])))
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
txt = "\n".join(out)
print(txt)
if len(sys.argv) > 2:
    open(sys.argv[2], "a").write(txt + "\n")
