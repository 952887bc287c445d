"""cgen_batch_augment on the GPU, through the C ABI and through data.DeviceDataset.batch: bit-exact against a CPU crop (F.pad with 0,
slice, flip on the u8 pixels, from the draws the kernel reports) pushed through the existing cgen_nchw_to_nhwc(src_is_u8 = 1) in the
same dtype; injected draws, 64-bit addressing, out-of-range rows, draw statistics and determinism, hipGraph capture."""
import ctypes as C
import math

import pytest
import torch

from augment_cases import CASES, CTX, INDEX, N, N_DATA, Case, make_args

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _lib_():
    from causal_gen_amd import _lib

    return _lib, _lib.require_gpu()


def _tdt(lib, dt):
    return torch.float32 if dt == "f32" else (torch.bfloat16 if lib.h16_is_bf16 else torch.float16)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _rng(seed=1234, offset=0):
    return torch.tensor([seed, offset], dtype=torch.int64, device=DEV)


def _nan_parent(lib, case, dt, n):
    return torch.full((case.view(n)[5],), float("nan"), dtype=_tdt(lib, dt), device=DEV)


def cpu_crop(data, index, draws, geom):
    """u8 NCHW batch for given (oy, ox, flip) rows; rows outside the data set stay all zero (= padding)."""
    h0, w0, r_h, r_w, px, py = geom
    out = torch.zeros((len(index), data.shape[1], r_h, r_w), dtype=torch.uint8)
    for b, (row, (oy, ox, flip)) in enumerate(zip(index, draws)):
        if not 0 <= row < data.shape[0]:
            continue
        img = torch.nn.functional.pad(data[row], (px, px, py, py))[:, oy:oy + r_h, ox:ox + r_w]
        out[b] = img.flip(-1) if flip else img
    return out


def expected_parent(_lib, lib, case, dt, batch_u8, n):
    """The NaN parent after the zero padding (if the view asks for it) and cgen_nchw_to_nhwc of the CPU batch."""
    sn, sh, sw, off, cpad, _ = case.view(n)
    par = _nan_parent(lib, case, dt, n)
    _, _, r_h, r_w, _, _ = case.geom
    if cpad:
        par.view(n, r_h, r_w, sw)[..., case.c:cpad] = 0
    src = batch_u8.to(DEV).contiguous()
    lib.nchw_to_nhwc(1, _lib.F32 if dt == "f32" else _lib.F16, n, case.c, r_h, r_w, src.data_ptr(),
                     _lib.View(par.data_ptr() + off * par.element_size(), sn, sh, sw, case.c, 0), 127.5, 1 / 127.5, _stream())
    torch.cuda.synchronize()
    return par


def run(_lib, lib, case, dt, data, index, pa=None, rng=None, draws_in=None, n_data=None):
    n = index.numel()
    par = _nan_parent(lib, case, dt, n)
    draws = torch.full((n, 3), -7, dtype=torch.int32, device=DEV)
    ctx = 0 if pa is None else pa.shape[1]
    pa_out = None if pa is None else torch.full((n, ctx), float("nan"), device=DEV)
    a = make_args(case, dt, data.data_ptr(), index.data_ptr(), par.data_ptr(), rng=None if rng is None else rng.data_ptr(),
                  draws_in=None if draws_in is None else draws_in.data_ptr(), draws_out=draws.data_ptr(),
                  pa_data=None if pa is None else pa.data_ptr(), pa_out=None if pa is None else pa_out.data_ptr(), n=n,
                  n_data=data.shape[0] if n_data is None else n_data, ctx=ctx)
    lib.batch_augment(C.byref(a), _stream())
    torch.cuda.synchronize()
    return par, draws, pa_out


@pytest.fixture(scope="module")
def sets():
    """One random u8 data set and parents per (c, h0, w0), shared by every test and never written."""
    g = torch.Generator().manual_seed(11)
    out = {}
    for cs in CASES:
        k = (cs.c,) + cs.geom[:2]
        if k not in out:
            out[k] = (torch.randint(0, 256, (N_DATA, cs.c) + cs.geom[:2], generator=g, dtype=torch.uint8), torch.randn(N_DATA, CTX, generator=g))
    return out


@pytest.mark.parametrize("dt", ["f32", "h16"])
@pytest.mark.parametrize("case", CASES, ids=[c.id() for c in CASES])
def test_exact_against_cpu_crop_through_the_layout_kernel(case, dt, sets):
    _lib, lib = _lib_()
    data, pa = sets[(case.c,) + case.geom[:2]]
    index = torch.tensor(INDEX, dtype=torch.int64, device=DEV)
    rng = _rng(99, 3)
    par, draws, pa_out = run(_lib, lib, case, dt, data.to(DEV), index, pa.to(DEV), rng)
    dr = draws.cpu().tolist()
    h0, w0, r_h, r_w, px, py = case.geom
    for oy, ox, flip in dr:
        assert 0 <= oy <= h0 + 2 * py - r_h and 0 <= ox <= w0 + 2 * px - r_w and flip in (0, 1), (oy, ox, flip)
    if case.hflip_p in (0.0, 1.0):
        assert all(d[2] == int(case.hflip_p) for d in dr)
    want = expected_parent(_lib, lib, case, dt, cpu_crop(data, list(INDEX), dr, case.geom), N)
    assert torch.equal(_bits(par), _bits(want))  # the view bit for bit, and every NaN around it untouched
    assert torch.equal(_bits(pa_out), _bits(pa.to(DEV)[index]))
    assert torch.equal(rng.cpu(), torch.tensor([99, 3]))  # the launch never advances the state


@pytest.mark.parametrize("dt", ["f32", "h16"])
@pytest.mark.parametrize("c", [1, 3])
def test_identity_geometry_equals_the_layout_kernel_on_the_data_set(c, dt, sets):
    _lib, lib = _lib_()
    case = Case(c, (8, 8, 8, 8, 0, 0), 0.0)
    data = sets[(c, 8, 8)][0]
    par, draws, _ = run(_lib, lib, case, dt, data.to(DEV), torch.arange(N_DATA, device=DEV), rng=_rng())
    assert draws.cpu().tolist() == [[0, 0, 0]] * N_DATA
    assert torch.equal(_bits(par), _bits(expected_parent(_lib, lib, case, dt, data, N_DATA)))


@pytest.mark.parametrize("dt", ["f32", "h16"])
def test_injected_draws_at_every_corner_are_used_and_echoed(dt, sets):
    _lib, lib = _lib_()
    for case in (Case(1, (5, 7, 6, 4, 2, 1), 0.5), Case(3, (28, 28, 32, 32, 4, 4), 0.5, "padded")):
        h0, w0, r_h, r_w, px, py = case.geom
        my, mx = h0 + 2 * py - r_h, w0 + 2 * px - r_w
        corners = [(oy, ox, f) for oy in (0, my) for ox in (0, mx) for f in (0, 1)]
        index = torch.tensor([i % N_DATA for i in range(len(corners))], dtype=torch.int64, device=DEV)
        d_in = torch.tensor(corners, dtype=torch.int32, device=DEV)
        data = sets[(case.c, h0, w0)][0]
        par, draws, _ = run(_lib, lib, case, dt, data.to(DEV), index, draws_in=d_in)  # (no Philox state at all)
        assert torch.equal(draws, d_in)
        want = expected_parent(_lib, lib, case, dt, cpu_crop(data, index.tolist(), corners, case.geom), len(corners))
        assert torch.equal(_bits(par), _bits(want))


def test_addressing_is_64_bit():
    """A data set of 60000 x 1 x 192 x 192 u8 = 2.2 GB; only the last row is initialised and indexed (byte offsets above 2^31)."""
    _lib, lib = _lib_()
    n_data, R = 60000, 192
    assert (n_data - 1) * R * R > 2 ** 31
    data = torch.empty((n_data, 1, R, R), dtype=torch.uint8, device=DEV)
    last = torch.randint(0, 256, (1, R, R), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    data[-1].copy_(last)
    case = Case(1, (R, R, R, R, 18, 9), 0.5)
    index = torch.tensor([n_data - 1], dtype=torch.int64, device=DEV)
    for dt in ("f32", "h16"):
        par, draws, _ = run(_lib, lib, case, dt, data, index, rng=_rng(7, 1))
        want = expected_parent(_lib, lib, case, dt, cpu_crop(last[None], [0], draws.cpu().tolist(), case.geom), 1)
        assert torch.equal(_bits(par), _bits(want))
    del data


@pytest.mark.parametrize("dt", ["f32", "h16"])
def test_out_of_range_rows_are_padding_and_never_read(dt, sets):
    _lib, lib = _lib_()
    case = Case(3, (5, 7, 6, 4, 2, 1), 0.5)
    data, pa = sets[(3, 5, 7)]
    index = torch.tensor([-1, N_DATA, 0], dtype=torch.int64, device=DEV)
    par, draws, pa_out = run(_lib, lib, case, dt, data.to(DEV), index, pa.to(DEV), _rng(3, 0))  # returns success (raises otherwise)
    dr = draws.cpu().tolist()
    assert dr[0] == dr[1] == [-1, -1, -1] and dr[2][0] >= 0
    # cpu_crop leaves rows outside the data set all zero = all padding value after normalisation
    want = expected_parent(_lib, lib, case, dt, cpu_crop(data, index.tolist(), dr, case.geom), 3)
    assert torch.equal(_bits(par), _bits(want))
    assert torch.equal(pa_out[:2], torch.zeros(2, CTX, device=DEV)) and torch.equal(_bits(pa_out[2]), _bits(pa.to(DEV)[0]))
    v = par.view(3, -1)[:2].float()
    assert torch.all(v == v[0, 0]) and abs(float(v[0, 0]) + 1.0) < 1e-3  # (0 - 127.5) / 127.5


def test_draw_statistics_determinism_and_row_keying():
    _lib, lib = _lib_()
    n = 4096
    case = Case(1, (4, 4, 4, 4, 2, 2), 0.5)
    data = torch.randint(0, 256, (n, 1, 4, 4), generator=torch.Generator().manual_seed(2), dtype=torch.uint8).to(DEV)
    index = torch.arange(n, device=DEV)
    rng = _rng(2024, 17)
    before = rng.clone()
    par, draws, _ = run(_lib, lib, case, "f32", data, index, rng=rng)
    assert torch.equal(rng, before)  # the Philox state is bit-identical after the launch
    d = draws.cpu()
    tol = 6 * math.sqrt(n * 0.2 * 0.8)
    for col in (0, 1):
        counts = torch.bincount(d[:, col], minlength=5)
        assert counts.numel() == 5 and all(abs(int(k) - n / 5) <= tol for k in counts), (col, counts.tolist())
    share = float(d[:, 2].float().mean())
    assert abs(share - 0.5) <= 6 * math.sqrt(0.25 / n), share
    # same state, same draws
    par2, draws2, _ = run(_lib, lib, case, "f32", data, index, rng=rng)
    assert torch.equal(draws, draws2) and torch.equal(_bits(par), _bits(par2))
    # a row's draw does not depend on its batch position or on the batch size
    perm = torch.roll(index, 5)  # row 4091 .. at position 0, row 0 at position 5
    _, draws_p, _ = run(_lib, lib, case, "f32", data, perm, rng=rng)
    assert torch.equal(draws_p, draws[perm])
    assert torch.equal(draws_p[5], draws[0])
    _, draws_1, _ = run(_lib, lib, case, "f32", data, index[:1].clone(), rng=rng)
    assert torch.equal(draws_1[0], draws[0])
    # the next state draws afresh
    lib.rng_advance(rng.data_ptr(), 1, _stream())
    _, draws3, _ = run(_lib, lib, case, "f32", data, index, rng=rng)
    assert int(rng[1]) == 18
    assert int((draws3 != draws).any(1).sum()) >= n // 2


@pytest.mark.parametrize("dt", ["f32", "h16"])
def test_captured_launch_draws_fresh_crops_on_every_replay(dt, sets):
    _lib, lib = _lib_()
    case = Case(1, (28, 28, 32, 32, 4, 4), 0.5, "padded")
    data, pa = sets[(1, 28, 28)]
    data_d, pa_d = data.to(DEV), pa.to(DEV)
    n = N
    rng = _rng(5, 0)
    index = torch.zeros(n, dtype=torch.int64, device=DEV)  # static buffers of the graph
    par = _nan_parent(lib, case, dt, n)
    draws = torch.zeros((n, 3), dtype=torch.int32, device=DEV)
    pa_out = torch.zeros((n, CTX), device=DEV)
    a = make_args(case, dt, data_d.data_ptr(), index.data_ptr(), par.data_ptr(), rng=rng.data_ptr(), draws_out=draws.data_ptr(),
                  pa_data=pa_d.data_ptr(), pa_out=pa_out.data_ptr(), n=n)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        st = _stream()
        lib.rng_advance(rng.data_ptr(), 1, st)
        lib.batch_augment(C.byref(a), st)
    got = []
    for rep, rows in enumerate(((0, 1, 2, 0, 1, 2, 0), (2, 2, 1, 0, 0, 1, 2))):
        index.copy_(torch.tensor(rows, dtype=torch.int64))
        g.replay()
        torch.cuda.synchronize()
        assert int(rng[1]) == rep + 1
        dr = draws.cpu().tolist()
        want = expected_parent(_lib, lib, case, dt, cpu_crop(data, list(rows), dr, case.geom), n)
        assert torch.equal(_bits(par), _bits(want))
        assert torch.equal(_bits(pa_out), _bits(pa_d[index]))
        got.append((par.clone(), dr))
    assert got[0][1] != got[1][1] and not torch.equal(_bits(got[0][0]), _bits(got[1][0]))


def test_device_dataset_batch_and_loader():
    from causal_gen_amd import DeviceDataset, DeviceLoader

    _lib, lib = _lib_()
    g = torch.Generator().manual_seed(8)
    n_data = 20
    x = torch.randint(0, 256, (n_data, 3, 28, 28), generator=g, dtype=torch.uint8)
    pa = torch.randn(n_data, 4, generator=g)
    ds = DeviceDataset(x, pa, 32, pad=(4, 4), hflip=0.5)
    index = torch.tensor([3, 19, 0, 3, 7], device=DEV)
    case = Case(3, (28, 28, 32, 32, 4, 4), 0.5)
    for dtype, dt in ((None, "f32"), (_tdt(lib, "h16"), "h16")):
        b = ds.batch(index, return_draws=True, dtype=dtype)
        assert tuple(b["x"].shape) == (5, 3, 32, 32) and b["x"].dtype == _tdt(lib, dt)
        assert b["x"].is_contiguous(memory_format=torch.channels_last)
        want = expected_parent(_lib, lib, case, dt, cpu_crop(x, index.tolist(), b["draws"].cpu().tolist(), case.geom), 5)
        assert torch.equal(_bits(b["x"].permute(0, 2, 3, 1).reshape(-1)), _bits(want))
        assert torch.equal(b["pa"], pa.to(DEV)[index])
        assert torch.equal(ds.reference_batch(index, b["draws"]), cpu_crop(x, index.tolist(), b["draws"].cpu().tolist(), case.geom))
        # the same draws injected reproduce the batch; the next training batch draws afresh
        again = ds.batch(index, draws=b["draws"], dtype=dtype)
        assert torch.equal(_bits(again["x"]), _bits(b["x"]))
    assert int(ds.rng[1]) == 2  # one advance per random training batch, none for the injected ones
    # evaluation: Pad(2), no flip, no randomness
    e = ds.batch(index, train=False, return_draws=True)
    assert e["draws"].cpu().tolist() == [[0, 0, 0]] * 5
    ref = (torch.nn.functional.pad(x[index.cpu()], (2, 2, 2, 2)).float() - 127.5) / 127.5
    torch.testing.assert_close(e["x"].cpu(), ref, rtol=0, atol=1e-6)
    with pytest.raises(ValueError, match="16-bit format"):
        ds.batch(index, dtype=torch.float64)
    ld = DeviceLoader(ds, 8, generator=torch.Generator(device=DEV).manual_seed(1))
    batches = list(ld)
    assert len(batches) == len(ld) == 2 and all(tuple(b["x"].shape) == (8, 3, 32, 32) and tuple(b["pa"].shape) == (8, 4) for b in batches)
    assert ld.last_perm.device.type == "cuda" and sorted(ld.last_perm.tolist()) == list(range(n_data))
