"""Device-resident input pipeline: the reference's train-time dataloader path (src/datasets.py: per-sample PIL
``RandomCrop(input_res, padding)`` + ``RandomHorizontalFlip(p)``, then a host-to-device copy and trainer.py:16-21's
``(x - 127.5) / 127.5``) for data sets that fit in HBM as u8 -- all four presets do, many times over.

The u8 images (at the data set's native resolution; ``TF.Resize`` belongs to data set preparation) and the f32 parents stay on
the device; ``cgen_batch_augment`` builds an augmented batch from a vector of row indices in ONE launch: row gather, zero-padded
random crop, horizontal flip, normalisation, NCHW -> NHWC, compute dtype, parents of the same rows.  The crop / flip draws come
from a device-side Philox state and are keyed by the DATA SET ROW (stream id 980), so a row's crop at a given state does not
depend on its batch position nor on the data-parallel rank that holds it, and a captured train step
(``TrainStep.step_from``) draws fresh crops on every replay without host work."""
import ctypes as C

import torch

from . import _lib

SUB, MUL = 127.5, 1.0 / 127.5  # trainer.py:17


def _pair(v):
    return (int(v), int(v)) if isinstance(v, (int, float)) else (int(v[0]), int(v[1]))


class DeviceDataset:
    """u8 images [N, c, h0, w0] and f32 parents [N, ctx], resident on `device`.

    ``pad = (pad_x, pad_y)`` is torchvision's ``padding=[left/right, top/bottom]`` of ``RandomCrop`` (value 0, applied to the u8
    pixels), ``input_res`` the crop size (int or (r_h, r_w)), ``hflip`` the flip probability.  A CPU `device` is allowed for
    host-side logic (geometry, loaders); building a batch needs the GPU."""

    def __init__(self, x_u8, pa, input_res, pad=(0, 0), hflip=0.5, device="cuda"):
        assert x_u8.dtype == torch.uint8 and x_u8.dim() == 4 and 1 <= x_u8.shape[1] <= 4, (x_u8.dtype, tuple(x_u8.shape))
        assert pa.dim() == 2 and pa.shape[0] == x_u8.shape[0], (tuple(pa.shape), tuple(x_u8.shape))
        self.device = torch.device(device)
        self.x = x_u8.to(self.device).contiguous()
        self.pa = pa.to(self.device, torch.float32).contiguous()
        self.device = self.x.device  # ("cuda" -> the concrete "cuda:0", comparable with the engine's)
        self.n_data, self.c, self.h0, self.w0 = (int(v) for v in self.x.shape)
        self.ctx = int(self.pa.shape[1])
        self.r_h, self.r_w = _pair(input_res)
        self.pad_x, self.pad_y = _pair(pad)
        self.hflip = float(hflip)
        if not 0.0 <= self.hflip <= 1.0:
            raise ValueError(f"hflip must lie in [0, 1] (got {hflip})")
        if self.pad_x < 0 or self.pad_y < 0 or self.r_h > self.h0 + 2 * self.pad_y or self.r_w > self.w0 + 2 * self.pad_x:
            raise ValueError(f"crop {self.r_h}x{self.r_w} does not fit the padded image "
                             f"{self.h0 + 2 * self.pad_y}x{self.w0 + 2 * self.pad_x}")
        self.rng = None  # own Philox state {seed, offset} of batch(); TrainStep.step_from uses the engine's instead

    @classmethod
    def from_args(cls, args, x_u8, pa, device="cuda"):
        """``args.pad`` / ``args.hflip`` per data set as src/datasets.py applies them: ukbb ``RandomCrop(padding=[2 * pad, pad])``
        + ``RandomHorizontalFlip(hflip)`` (:107-118), morphomnist / cmnist ``RandomCrop(32, padding=pad)`` without a flip
        (:284, :371), mimic no augmentation (:513-519)."""
        name = str(getattr(args, "dataset", "") or "") + " " + str(getattr(args, "hps", ""))
        p = int(getattr(args, "pad", 0) or 0)
        if "ukbb" in name:
            pad, hflip = (2 * p, p), float(getattr(args, "hflip", 0.5))
        elif "mnist" in name:
            pad, hflip = (p, p), 0.0
        elif "mimic" in name:
            pad, hflip = (0, 0), 0.0
        else:
            raise ValueError(f"no augmentation recipe for data set / preset {name.strip()!r}")
        return cls(x_u8, pa, int(args.input_res), pad=pad, hflip=hflip, device=device)

    def __len__(self):
        return self.n_data

    def geometry(self, train=True):
        """(r_h, r_w, pad_x, pad_y, hflip_p) of the train transform, or of the evaluation one: no flip, centred padding
        ((R - w0) // 2, (R - h0) // 2) with a zero draw range -- ``Pad(2)`` for the 28x28 digits, the identity for ukbb."""
        if train:
            return self.r_h, self.r_w, self.pad_x, self.pad_y, self.hflip
        if self.r_h < self.h0 or self.r_w < self.w0 or (self.r_h - self.h0) % 2 or (self.r_w - self.w0) % 2:
            raise ValueError(f"evaluation pads {self.h0}x{self.w0} symmetrically up to {self.r_h}x{self.r_w}: not possible")
        return self.r_h, self.r_w, (self.r_w - self.w0) // 2, (self.r_h - self.h0) // 2, 0.0

    def draw_range(self, train=True):
        """(max oy, max ox): the offsets are uniform on [0, max]."""
        r_h, r_w, px, py, _ = self.geometry(train)
        return self.h0 + 2 * py - r_h, self.w0 + 2 * px - r_w

    def key(self, train=True):
        """Identity + geometry: what a captured launch bakes in."""
        return (id(self), self.x.data_ptr(), self.pa.data_ptr(), self.n_data, self.c, self.h0, self.w0, self.ctx) + self.geometry(train)

    def args_for(self, dt, n, index_ptr, out_view, rng_ptr, train=True, draws_in=None, draws_out=None, pa_out=None):
        """The ``cgen_augment_args`` of one launch (pointers as integers; `out_view` a ``_lib.View``)."""
        r_h, r_w, px, py, p = self.geometry(train)
        a = _lib.AugmentArgs()
        a.dtype, a.n, a.c, a.h0, a.w0, a.r_h, a.r_w, a.pad_x, a.pad_y = dt, n, self.c, self.h0, self.w0, r_h, r_w, px, py
        a.ctx, a.stream_id, a.hflip_p, a.sub, a.mul, a.n_data = self.ctx, _lib.STREAM_AUGMENT, p, SUB, MUL, self.n_data
        a.data, a.index, a.out, a.rng = self.x.data_ptr(), index_ptr, out_view, rng_ptr
        a.draws_in, a.draws_out = draws_in, draws_out
        a.pa_data, a.pa_out = (self.pa.data_ptr(), pa_out) if pa_out else (None, None)
        return a

    def _own_rng(self):
        if self.rng is None:
            self.rng = torch.tensor([torch.initial_seed() & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64, device=self.device)
        return self.rng

    def planar_view(self, ptr, train=True):
        """The ``cgen_view`` that tells ``cgen_batch_augment_planar`` its output is a contiguous f32 [n, c, r_h, r_w] at `ptr`."""
        r_h, r_w, _, _, _ = self.geometry(train)
        return _lib.View(ptr, self.c * r_h * r_w, r_w, 1, self.c, 0)

    def batch(self, index, train=True, draws=None, return_draws=False, dtype=None, rng=None, planar=False):
        """{"x", "pa"} for the rows `index` (device int64 vector): ``x`` has NCHW shape over NHWC memory (the f32 engine takes it
        zero-copy, engine.from_nchw's channels-last branch), in `dtype` (f32, or the library's 16-bit storage format).
        `planar`: ``x`` is a contiguous f32 NCHW tensor instead (``cgen_batch_augment_planar``: what the anticausal predictors
        read), the same values bit for bit.
        `draws` (int32 [n, 3] of (oy, ox, flip)) overrides the random draws; `return_draws` adds the ones used as "draws".
        `rng`: a device int64 {seed, offset} tensor to draw from as it stands; by default the data set's own state, moved on by
        one per training batch (the launch itself never advances a state)."""
        lib = _lib.require_gpu()
        index = index.to(self.device, torch.int64).contiguous()
        n = int(index.numel())
        dtype = torch.float32 if dtype is None else dtype
        h16 = torch.bfloat16 if lib.h16_is_bf16 else torch.float16
        if dtype not in (torch.float32, h16):
            raise ValueError(f"dtype must be torch.float32 or {h16} (the library's 16-bit format), got {dtype}")
        if planar and dtype != torch.float32:
            raise ValueError(f"the planar batch is f32 (got {dtype})")
        r_h, r_w, _, _, _ = self.geometry(train)
        st = torch.cuda.current_stream(self.device).cuda_stream
        out = torch.empty((n, self.c, r_h, r_w) if planar else (n, r_h, r_w, self.c), dtype=dtype, device=self.device)
        pa = torch.empty((n, self.ctx), dtype=torch.float32, device=self.device)
        d_in = None
        if draws is not None:
            d_in = draws.to(self.device, torch.int32).contiguous()
            assert tuple(d_in.shape) == (n, 3), tuple(d_in.shape)
        elif rng is None:
            rng = self._own_rng()
            if train:
                lib.rng_advance(rng.data_ptr(), 1, st)
        d_out = torch.empty((n, 3), dtype=torch.int32, device=self.device) if return_draws else None
        view = self.planar_view(out.data_ptr(), train) if planar else _lib.View(out.data_ptr(), r_h * r_w * self.c, r_w * self.c, self.c, self.c, 0)
        a = self.args_for(_lib.F32 if dtype == torch.float32 else _lib.F16, n, index.data_ptr(), view,
                          None if rng is None else rng.data_ptr(), train, None if d_in is None else d_in.data_ptr(),
                          None if d_out is None else d_out.data_ptr(), pa.data_ptr())
        (lib.batch_augment_planar if planar else lib.batch_augment)(C.byref(a), st)
        res = {"x": out if planar else out.permute(0, 3, 1, 2), "pa": pa}
        if return_draws:
            res["draws"] = d_out
        return res

    def reference_batch(self, index, draws, train=True):
        """The same batch built with torch ops on the CPU from given draws, as u8 NCHW (F.pad with 0, slice, flip): what the
        reference's transforms produce for these offsets.  For tests and for reproducing a batch; not a product path."""
        r_h, r_w, px, py, _ = self.geometry(train)
        x = self.x.cpu()
        idx, dr = index.cpu().tolist(), draws.cpu().tolist()
        out = torch.zeros((len(idx), self.c, r_h, r_w), dtype=torch.uint8)
        for b, (row, (oy, ox, flip)) in enumerate(zip(idx, dr)):
            if not 0 <= row < self.n_data:
                continue
            img = torch.nn.functional.pad(x[row], (px, px, py, py))[:, oy:oy + r_h, ox:ox + r_w]
            out[b] = img.flip(-1) if flip else img
        return out


class DeviceLoader:
    """Epochs of index vectors over a :class:`DeviceDataset`: one permutation per epoch, drawn on the data set's device from
    `generator` (default: a generator of that device seeded with ``torch.initial_seed()``).  Under data parallelism every rank
    builds the loader with the same seed, so all ranks hold the SAME permutation (as ``dp.shared_categorical_draw`` shares its
    draw: by the common seed, no collective) and rank r takes the r-th contiguous shard of each global batch of
    ``batch_size * world_size`` rows.  Iterating yields ``ds.batch(...)``; :meth:`indices` yields the index vectors alone
    (for ``TrainStep.step_from``)."""

    def __init__(self, ds, batch_size, shuffle=True, drop_last=True, train=True, generator=None, rank=0, world_size=1):
        if world_size > 1 and not drop_last:
            raise ValueError("data-parallel ranks must run the same number of equal steps: drop_last=True")
        assert 0 <= rank < world_size and batch_size > 0
        self.ds, self.batch_size, self.shuffle, self.drop_last, self.train = ds, int(batch_size), shuffle, drop_last, train
        self.rank, self.world = int(rank), int(world_size)
        if generator is None and shuffle:
            generator = torch.Generator(device=ds.device)
            generator.manual_seed(torch.initial_seed())
        self.generator = generator
        self.last_perm = None

    def __len__(self):
        g = self.batch_size * self.world
        return len(self.ds) // g if self.drop_last else (len(self.ds) + g - 1) // g

    def indices(self):
        n, g = len(self.ds), self.batch_size * self.world
        perm = (torch.randperm(n, device=self.ds.device, generator=self.generator) if self.shuffle
                else torch.arange(n, device=self.ds.device))
        self.last_perm = perm
        for i in range(len(self)):
            glob = perm[i * g:(i + 1) * g]
            yield glob[self.rank * self.batch_size:(self.rank + 1) * self.batch_size]

    def __iter__(self):
        for idx in self.indices():
            yield self.ds.batch(idx, train=self.train)


class AugmentedInput:
    """Stands in for the image tensor of a train step (HVAE._run_forward / _prep_inputs): ``emit(eng)`` launches
    ``cgen_batch_augment`` straight into a fresh engine tensor in the compute dtype -- zero padding channels included, so no fill
    and no conversion pass follow -- and into the static parents buffer `pa_buf`, reading the static index buffer `index_buf`
    (both have stable addresses: a captured step replays with whatever they hold) and the engine's Philox state."""

    def __init__(self, ds, n, train=True, draws_out=None):
        self.ds, self.n, self.train = ds, int(n), train
        r_h, r_w, _, _, _ = ds.geometry(train)
        self.shape = (self.n, ds.c, r_h, r_w)
        self.dtype = torch.uint8
        self.index_buf = torch.zeros(self.n, dtype=torch.int64, device=ds.device)
        self.pa_buf = torch.zeros((self.n, ds.ctx), dtype=torch.float32, device=ds.device)
        self.draws_out = draws_out
        if draws_out is not None:
            assert draws_out.dtype == torch.int32 and tuple(draws_out.shape) == (self.n, 3) and draws_out.is_contiguous()
        self.key = ("augment", ds.key(train), None if draws_out is None else draws_out.data_ptr())

    def dim(self):
        return 4

    def load(self, index):
        assert index.dtype == torch.int64 and index.numel() == self.n, (index.dtype, tuple(index.shape))
        if index.data_ptr() != self.index_buf.data_ptr():
            self.index_buf.copy_(index.reshape(-1), non_blocking=True)

    def emit(self, eng):
        ds = self.ds
        assert eng.device == ds.device, (eng.device, ds.device)
        n, c, r_h, r_w = self.shape
        out = eng.new(n, r_h, r_w, c, rg=False)
        out.keep = self
        if c % 8:
            out.cpad = out.sw  # the launch writes the zero padding up to the 8-channel pixel stride itself
        a = ds.args_for(eng.dt, n, self.index_buf.data_ptr(), out.cv(), eng.rng_ptr(), self.train, None,
                        None if self.draws_out is None else self.draws_out.data_ptr(), self.pa_buf.data_ptr())
        eng.lib.batch_augment(C.byref(a), eng.stream)
        eng.launches += 1
        return out
