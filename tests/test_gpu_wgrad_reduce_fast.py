"""cgen_wgrad_reduce_tiles (csrc/multitensor.hip: a tile of a site per workgroup, the four split chains on different lanes, the OIHW
gradient written from LDS in runs) against the per-element reference kernel behind cgen_wgrad_reduce_ref: equal BITS in grad_w and
grad_b on random partials.  Both partial layouts, ks 1 / 3 / 7, every split count at which the chain batches of the reference change
(1, 3, 4, 5, 16, 17, 37, 144; 2048 as in the real step), accumulate on a non-zero gradient, unscale 0 and 2^-12, with and without bias,
weight counts that are no multiple of 4 (the plain-order path, bias elements starting inside a thread's four), rows that need more than one tile, several
sites in one launch, guard bands behind every gradient."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64  # floats

# (layout, ks, co, ci, nsplit, bias)
SITES = [
    (0, 1, 8, 4, 1, 1), (1, 3, 20, 24, 1, 1), (0, 3, 32, 36, 3, 0), (1, 7, 8, 4, 3, 1), (0, 7, 32, 1, 4, 1), (1, 1, 132, 64, 4, 1),
    (0, 3, 132, 24, 5, 1), (1, 3, 8, 64, 5, 0), (0, 1, 132, 64, 16, 1), (1, 3, 16, 32, 16, 1), (0, 3, 20, 4, 17, 1), (1, 7, 8, 4, 17, 1),
    (0, 7, 32, 1, 37, 1), (1, 1, 32, 36, 37, 0), (0, 3, 8, 32, 144, 1), (1, 3, 8, 64, 144, 1),
    (0, 3, 64, 96, 5, 1),   # 55 296 elements: many tiles
    (0, 3, 4, 256, 3, 1),   # a partial row block wider than a tile: cut along ci
    (1, 3, 300, 8, 4, 1),   # layout 1 cut along co
    (0, 3, 2, 6, 4, 1), (1, 3, 6, 2, 5, 1),  # the four-chain order, but no 16-byte loads (inner dimension 6)
    (0, 3, 3, 5, 1, 1), (0, 3, 3, 5, 5, 1), (0, 3, 3, 5, 17, 1), (1, 3, 5, 3, 4, 1), (0, 1, 7, 9, 37, 1), (1, 7, 3, 3, 144, 1),  # weight count % 4 != 0
    (0, 3, 8, 8, 2048, 1), (1, 3, 8, 8, 2048, 0),  # what the 192x192 layers leave in the step: 512 splits per chain
    (0, 3, 41, 25, 16, 1),  # 9 225 weights: the bias starts in the middle of a thread's four and of a 1 024-chunk
]


def _run(lib, entry, sites, parts, grads0, accumulate, unscale):
    from causal_gen_amd import _lib
    from causal_gen_amd.wgrad_sched import plan_wred_items

    grads = grads0.clone()
    descs, off = [], 0
    for (layout, ks, co, ci, nsplit, bias), part in zip(sites, parts):
        nw = co * ci * ks * ks
        d = _lib.WredDesc()
        d.partial_w = part.data_ptr()
        d.partial_b = part.data_ptr() + 4 * nsplit * nw if bias else None
        d.grad_w = grads.data_ptr() + 4 * off
        off += nw + GUARD
        d.grad_b = grads.data_ptr() + 4 * off if bias else None
        off += co + GUARD
        d.co, d.ci_total, d.ks, d.nsplit, d.accumulate, d.unscale, d.layout = co, ci, ks, nsplit, accumulate, unscale, layout
        d.numel = nw + (co if bias else 0)
        descs.append(d)
    if entry == "ref":
        csite, cidx = [], []
        for i, d in enumerate(descs):
            nch = (d.numel + 1023) // 1024
            csite += [i] * nch
            cidx += list(range(nch))
        arr = (_lib.WredDesc * len(descs))(*descs)
        dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
        cs = torch.tensor(csite, dtype=torch.int32, device="cuda")
        cx = torch.tensor(cidx, dtype=torch.int32, device="cuda")
        lib.wgrad_reduce_ref(dev.data_ptr(), cs.data_ptr(), cx.data_ptr(), len(csite), None)
    else:
        items = plan_wred_items(descs)
        dev = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).cuda()
        lib.wgrad_reduce_tiles(dev.data_ptr(), len(items), None)
    torch.cuda.synchronize()
    return grads.cpu()


@pytest.fixture(scope="module")
def problem():
    g = torch.Generator().manual_seed(23)
    parts, total = [], 0
    for layout, ks, co, ci, nsplit, bias in SITES:
        nw = co * ci * ks * ks
        # magnitudes spread over 2^12 so that the order of the additions shows in the last bits
        p = torch.randn(nsplit * (nw + co), generator=g) * torch.exp2(torch.randint(-6, 7, (nsplit * (nw + co),), generator=g).float())
        parts.append(p.cuda())
        total += nw + co + 2 * GUARD
    grads0 = torch.randn(total, generator=g).cuda()
    return parts, grads0


@pytest.mark.parametrize("accumulate,unscale", [(0, 0.0), (1, 2.0 ** -12), (0, 2.0 ** -12), (1, 0.0)])
def test_tiled_reduce_has_the_reference_bits(problem, accumulate, unscale):
    from causal_gen_amd import _lib

    lib = _lib.require_gpu()
    parts, grads0 = problem
    want = _run(lib, "ref", SITES, parts, grads0, accumulate, unscale)
    got = _run(lib, "tiles", SITES, parts, grads0, accumulate, unscale)
    g0 = grads0.cpu()
    assert not torch.equal(want.view(torch.int32), g0.view(torch.int32))
    off = 0
    for site in SITES:
        layout, ks, co, ci, nsplit, bias = site
        nw = co * ci * ks * ks
        for n, is_bias in ((nw, False), (co, True)):
            a, b = want[off:off + n].view(torch.int32), got[off:off + n].view(torch.int32)
            if is_bias and not bias:
                assert torch.equal(b, g0[off:off + n].view(torch.int32)), site
            else:
                assert torch.equal(a, b), (site, "bias" if is_bias else "weight", int((a != b).sum()), n)
            for t in (want, got):  # the guard band behind it is untouched
                assert torch.equal(t[off + n:off + n + GUARD].view(torch.int32), g0[off + n:off + n + GUARD].view(torch.int32)), site
            off += n + GUARD
    assert off == grads0.numel()
