"""Every idle gap (no kernel resident) in the FORWARD pass of the last graph-replayed train step of a rocprofv3 kernel trace (csv),
one line each: where it sits, how long, the kernel that ended before it and the one that started after it, and whether the two
share a queue.  The decoder's gaps are labelled with the layer's resolution (counted from the upsample launches: a new resolution
begins with the first upsample behind a latent tail) and summed per (resolution, kernel before -> kernel after); the sum over the
resolutions named with --served is the idle time a forward pair launch of those layers could remove at most.
Same step selection as tools/timeline.py (the shortest whole step = a graph replay).
usage: python tools/fwd_gaps.py <kernel_trace.csv> [out.txt] [--res 1,6,12,24,48,96,192] [--served 6,12,24,48]"""
import collections
import csv
import re
import sys

args = [a for a in sys.argv[1:]]
res_list, served = [1, 6, 12, 24, 48, 96, 192], [6, 12, 24, 48]
for flag in ("--res", "--served"):
    if flag in args:
        k = args.index(flag)
        vals = [int(v) for v in args[k + 1].split(",")]
        del args[k:k + 2]
        if flag == "--res":
            res_list = vals
        else:
            served = vals

rows = []
with open(args[0]) as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Queue_Id", ""),
                     int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"]))))
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
fin = next(k for k, r in enumerate(step) if "elbo_finalize" in r[2])
fwd = step[:fin + 1]
t0 = fwd[0][0]


def short(n):
    n = re.sub(r"^void ", "", n)
    n = re.sub(r"\(.*$", "", n)
    return n.replace("cgen::", "").replace("unsigned short", "u16")[:40]


def fam(n):
    return re.sub(r"<.*$", "", short(n))


# resolution of every launch: index into res_list = number of upsample groups begun so far
res_of, idx, tail_since = [], 0, True
dec_start = None
for k, r in enumerate(fwd):
    n = r[2]
    if "upsample_fwd" in n:
        if tail_since:
            idx += 1
            tail_since = False
    elif "latent_tail" in n or "reparam_kl_fwd" in n:
        tail_since = True
        if dec_start is None:
            dec_start = k
    res_of.append(res_list[min(idx, len(res_list) - 1)])
# the decoder begins with the 1x1 layers' Blocks, a few launches in front of the first latent tail: take the first tail as its start
out = []
P = out.append
gaps = []
cur_e, cur = fwd[0][1], 0
for k in range(1, len(fwd)):
    s, e = fwd[k][0], fwd[k][1]
    if s > cur_e:
        gaps.append((k, cur, s - cur_e))
    if e > cur_e:
        cur_e, cur = e, k
P("forward pass: %d launches, %.3f ms (start .. elbo_finalize end); idle %.1f us in %d gaps"
  % (len(fwd), (fwd[fin][1] - t0) / 1e6, sum(g[2] for g in gaps) / 1e3, len(gaps)))
P("at us | gap us | part | kernel before (workgroups) -> kernel after (workgroups) | queues")
acc = collections.OrderedDict()
for k, c, g in gaps:
    part = "encoder" if dec_start is None or k < dec_start else "dec %3d" % res_of[k]
    same = "same queue" if fwd[k][3] == fwd[c][3] else "other queue"
    P("%9.1f | %5.2f | %s | %s (%d) -> %s (%d) | %s" % ((fwd[k][0] - t0) / 1e3, g / 1e3, part, short(fwd[c][2]), fwd[c][4],
                                                      short(fwd[k][2]), fwd[k][4], same))
    a = acc.setdefault((part, fam(fwd[c][2]), fam(fwd[k][2]), same), [0, 0])
    a[0] += 1
    a[1] += g
P("grouped:")
for (part, a_, b_, same), (cnt, g) in acc.items():
    P("  %s  %-26s -> %-26s %-11s x%-3d %7.1f us  avg %5.2f" % (part, a_, b_, same, cnt, g / 1e3, g / 1e3 / cnt))
per = collections.OrderedDict()
for k, c, g in gaps:
    part = "encoder" if dec_start is None or k < dec_start else res_of[k]
    a = per.setdefault(part, [0, 0])
    a[0] += 1
    a[1] += g
P("per part: " + "   ".join("%s: %d gaps %.1f us" % (str(p), c, g / 1e3) for p, (c, g) in per.items()))
tot = sum(g for p, (c, g) in per.items() if p in served)
cnt = sum(c for p, (c, g) in per.items() if p in served)
P("decoder layers at %s: %d gaps, %.1f us idle" % (", ".join("%d^2" % r for r in served), cnt, tot / 1e3))
# the Blocks and tails of the decoder per resolution: mean duration, and how much of each side-queue launch overlaps the main queue's
mainq = fwd[fin][3]
blk = collections.OrderedDict()
for k, r in enumerate(fwd):
    if dec_start is None or k < dec_start - 8:
        continue
    if any(t in r[2] for t in ("blk3", "blk4", "latent_tail", "upsample_fwd")):
        a = blk.setdefault((res_of[k], short(r[2]), r[4], "main" if r[3] == mainq else "side"), [0, 0])
        a[0] += 1
        a[1] += r[1] - r[0]
P("decoder launches per resolution: res | kernel | workgroups | queue | count | mean us")
for (rs, n, wg, q), (cnt, d) in blk.items():
    P("  %3d | %-40s | %5d | %s | x%-3d | %6.1f" % (rs, n, wg, q, cnt, d / 1e3 / cnt))
txt = "\n".join(out)
print(txt)
if len(args) > 1:
    open(args[1], "w").write(txt + "\n")
