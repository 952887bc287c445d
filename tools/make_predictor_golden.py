"""Generate tests/golden/predictor_{morphomnist,cmnist}.pt from the REFERENCE's own ``layers.CNN`` (src/pgm/layers.py), run on the
CPU in eval mode, in f64 and in f32.  Build-machine tool: it reads the reference tree; no GPU test does.

``layers.py`` imports pyro at module level; the predictor CNN itself is plain torch, so stub modules stand in for pyro.  Weights
and BatchNorm running statistics are drawn at random and rounded to binary16-representable values, stored as f16 (exact).
Inputs include a constant background and +-1-clamped regions (what cf_x looks like after dscm.py:55-56).  Stored per head: the
state dict, the context, the f64 / f32 outputs, and d(sum(wout * out))/dx in f64."""
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("CGEN_REFERENCE_SRC", "/root/reference/src")
sys.path[:0] = [os.path.join(REF, "pgm"), REF]

import torch  # noqa: E402


class _Any(types.ModuleType):
    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return type(k, (object,), {"__init__": lambda self, *a, **kw: None})


for _m in ("pyro", "pyro.infer", "pyro.distributions", "pyro.distributions.conditional", "pyro.distributions.torch_distribution",
           "pyro.nn", "pyro.distributions.transforms"):
    sys.modules.setdefault(_m, _Any(_m))
    if "." in _m:
        _parent, _, _leaf = _m.rpartition(".")
        setattr(sys.modules[_parent], _leaf, sys.modules[_m])

import layers as ref_layers  # noqa: E402  (reference: src/pgm/layers.py)

PRESETS = {
    # tag: (in_shape, B, [(encoder name, width, num_outputs, context_dim)])
    "morphomnist": ((1, 32, 32), 5, [("encoder_t", 8, 2, 1), ("encoder_i", 8, 2, 0), ("encoder_y", 8, 10, 0)]),
    "cmnist": ((3, 32, 32), 3, [("encoder_y", 8, 10, 0), ("encoder_c", 8, 10, 0)]),
    # FlowPGM's four image heads (default width 16): stride-2 7x7, max-pool.  One file per head keeps each under 1 MiB.
    "ukbb192": ((1, 192, 192), 1, [("encoder_v", 16, 2, 0), ("encoder_b", 16, 2, 1), ("encoder_s", 16, 1, 1), ("encoder_m", 16, 1, 0)]),
}
SPLIT = {"ukbb192"}


def f16_round(t):
    return t.half().float()


def randomise(cnn, g):
    with torch.no_grad():
        for name, p in cnn.named_parameters():
            fan = p[0].numel() if p.dim() > 1 else 1
            if p.dim() > 1:
                v = torch.randn(p.shape, generator=g) * (1.6 / fan ** 0.5)
            elif name.endswith("weight"):
                v = 0.7 + 0.6 * torch.rand(p.shape, generator=g)
            else:
                v = 0.1 * torch.randn(p.shape, generator=g)
            p.copy_(f16_round(v))
        for name, b in cnn.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(f16_round(0.2 * torch.randn(b.shape, generator=g)))
            elif name.endswith("running_var"):
                b.copy_(f16_round(0.5 + torch.rand(b.shape, generator=g)))


def make_x(shape, B, g):
    C, R, _ = shape
    x = (torch.rand(B, C, R, R, generator=g) * 2 - 1) * 1.3
    x = (x.clamp(-1, 1) * 256).round() / 256  # +-1 plateaus where |.| > 1; on a 1/256 grid (binary16-exact)
    x[0, :, : R // 2, :] = -1.0  # constant background
    x[:, :, :, : R // 8] = -1.0
    return x


def run(tag, seed=0):
    shape, B, heads = PRESETS[tag]
    g = torch.Generator().manual_seed(seed)
    x = make_x(shape, B, g)
    out = {"in_shape": shape, "x": x, "heads": {}}
    for name, width, nout, ctx in heads:
        cnn = ref_layers.CNN(shape, width=width, num_outputs=nout, context_dim=ctx)
        randomise(cnn, g)
        cnn.eval()
        y = torch.rand(B, ctx, generator=g) * 2 - 1 if ctx else None
        wout = torch.randn(B, nout, generator=g)
        c64 = cnn.double()
        x64 = x.double().requires_grad_(True)
        o64 = c64(x64, y.double() if y is not None else None)
        (gx,) = torch.autograd.grad((o64 * wout.double()).sum(), x64)
        with torch.no_grad():
            o32 = cnn.float()(x, y)
        sd = {k: (v.half() if v.is_floating_point() else v) for k, v in cnn.state_dict().items()}
        out["heads"][name] = {"width": width, "nout": nout, "ctx": ctx, "state_dict": sd, "y": y, "out64": o64.detach(),
                              "out32": o32, "wout": wout, "gx64": gx.float()}
    return out


if __name__ == "__main__":
    dst = os.path.join(ROOT, "tests", "golden")
    for tag in PRESETS:
        res = run(tag)
        if tag not in SPLIT:
            parts = {tag: res}
        else:  # x stored once per file as binary16 (exact on its grid)
            parts = {f"{tag}_{name}": dict(res, x=res["x"].half(), heads={name: h}) for name, h in res["heads"].items()}
        for ptag, part in parts.items():
            path = os.path.join(dst, f"predictor_{ptag}.pt")
            torch.save(part, path)
            print(path, os.path.getsize(path))
