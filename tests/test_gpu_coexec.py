"""Every instance of the fused light-Block kernel (csrc/block.hip) must give the same bits beside a packed weight-gradient batch as
alone: with CGEN_WGRAD_BG_SERIAL=0 the engine's flush (wgrad_sched.py) runs exactly such a batch on a second stream beside the
backward chain.

tools/coexec_probe.py replays the forward and the data-gradient launch of one Block on fixed seeded inputs, 100 times each, while one
`cgen_conv2d_wgrad_batch_run` batch with the flush's 304-workgroup cap (copies of a 64 -> 16 3x3 problem at 96^2, B = 32, ~340 us:
it outlasts every victim) runs on a second stream, and compares every byte of the pass's arena with the same launch alone.  It runs
ONCE, in a process of its own, for all cases: which instance a launch took is read from the kernel's own trace (CGEN_CONV_TRACE),
and that switch is read once per process at the first launch.

On the parent commit the five B = 32 cases passed (0 of 100 each: a stale read is too rare there -- about one launch of the 12x12
data gradient in a few thousand at eight times the batch) and the last case FAILED: 6 of 4000 launches of the 12x12 data gradient at
B = 256 differed, because wave 7 of `blk3s_kernel<false>` reached the first barrier without having waited for its own pieces of the
input tile (LABNOTES 12).  With the wait in place: 0 of 4000."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (case of tools/coexec_probe.py, trace line of the instance it must take: forward and data gradient)
CASES = [
    ("blk3s6", r"blk3s\[%s\] 32x6x6 ctot8 160 b 40 Co 160 "),
    ("blk3s12", r"blk3s\[%s\] 32x12x12 ctot8 160 b 40 Co 160 "),
    ("blk3_24", r"blk3\[%s\] 32x24x24 ctot8 128 b 32 Co 128 .* tile rows 8$"),
    ("blk3_48", r"blk3\[%s\] 32x48x48 ctot8 96 b 24 Co 96 .* tile rows 12$"),
    ("blk3r96", r"blk3r\[%s\] 32x96x96 c 64 b 16 Co 64 "),
    # the form in which the missing wait of the small-image data gradient showed within seconds (see above)
    ("blk3s12:256:4000:bwd", r"blk3s\[%s\] 256x12x12 ctot8 160 b 40 Co 160 "),
]


@pytest.fixture(scope="module")
def probed():
    env = dict(os.environ, CGEN_CONV_TRACE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "coexec_probe.py"), "--cases", ",".join(c for c, _ in CASES)],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 1), (r.returncode, r.stderr[-3000:])  # (1: a launch differed -- reported per case below)
    res = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("{"):
            d = json.loads(ln)
            res[d["spec"]] = d
    return res, set(r.stderr.splitlines())


@pytest.mark.parametrize("case,trace", CASES, ids=[c for c, _ in CASES])
def test_fused_block_is_bit_identical_beside_a_packed_weight_gradient_batch(probed, case, trace):
    res, lines = probed
    assert case in res, sorted(res)
    d = res[case]
    dirs = [k for k in ("fwd", "bwd") if k + "_reps_differing" in d]
    assert dirs == (["bwd"] if case.endswith(":bwd") else ["fwd", "bwd"])
    for k in dirs:
        print(case, k, "launches differing:", d[k + "_reps_differing"], "of", d["reps"], "| alone", d[k + "_alone_us"], "us, batch", d["wgrad_batch_us"], "us")
        assert any(re.match(trace % k, ln) for ln in lines), ("the case did not take the instance it names", case, k, [ln for ln in lines if ln.startswith("blk3")][:6])
        assert d[k + "_alone_us"] < d["wgrad_batch_us"], "the batch must outlast the victim"
        assert d[k + "_reps_differing"] == 0, (case, k, d)
