"""Seeded parent SCMs and observation batches shared by tests/test_pgm_logprob.py (host density, f64) and
tests/test_gpu_pgm_train.py (kernel against the host density).  Nothing here needs a GPU."""
import copy
from types import SimpleNamespace

import torch
import torch.nn.functional as F

KINDS = ("flow", "morpho", "colour", "chest")


def make_pgm(kind, seed=0, widths=None, scale=0.3):
    """A PGM of `kind` whose every parameter is its initial value plus `scale` * N(0, 1) from a seeded generator (f32)."""
    from causal_gen_amd import pgm as P

    cls = {"flow": P.FlowPGM, "morpho": P.MorphoMNISTPGM, "colour": P.ColourMNISTPGM, "chest": P.ChestPGM}[kind]
    torch.manual_seed(1000 + seed)
    m = cls(SimpleNamespace(widths=list(widths)) if widths else SimpleNamespace())
    g = torch.Generator().manual_seed(2000 + seed)
    linear = {id(mod.weight): mod.in_features for mod in m.modules() if isinstance(mod, torch.nn.Linear)}
    with torch.no_grad():
        for p in m.parameters():
            # (a Linear weight moves by scale / sqrt(fan-in), so that a [64, 64, 64] network keeps O(1) outputs)
            p.add_(scale / linear.get(id(p), 1) ** 0.5 * torch.randn(p.shape, generator=g))
    return m


def draw(m, n, seed=0):
    """`n` rows drawn from the model itself (f32)."""
    return m.sample(n, generator=torch.Generator().manual_seed(3000 + seed))


def cast(obs, dtype):
    return {k: v.to(dtype) for k, v in obs.items()}


def to64(m):
    """An f64 CPU copy of the same parameters."""
    return copy.deepcopy(m).cpu().double()


def spline_of(m):
    from causal_gen_amd.pgm import LinearSpline

    return next((mod for mod in m.modules() if isinstance(mod, LinearSpline)), None)


def spline_var(m):
    return next((mech for mech in m.mechanisms() if mech.kind == "spline"), None)


def edge_rows(m, obs, kind):
    """`obs` with its first rows overwritten by edge cases, where the PGM has the mechanism: a spline input at exactly +-bound and
    outside the bound (the spline is the identity there and its parameters get nothing from the row); every `finding` 0; class 9
    of `digit` absent."""
    obs = {k: v.clone() for k, v in obs.items()}
    sp, mech = spline_of(m), spline_var(m)
    if sp is not None and not mech.normalize:
        b = float(sp.bound)
        vals = torch.tensor([b, -b, b + 0.5, -b - 1.25, 7.0])
        obs[mech.var][:len(vals), 0] = vals
    if kind == "chest":
        obs["finding"].zero_()
    if "digit" in obs:
        d = obs["digit"].argmax(-1)
        d[d == 9] = 3
        obs["digit"] = F.one_hot(d, 10).float()
    return obs


def clamp_rows(m):
    """Eight Morpho-MNIST rows with thickness, then intensity, at +-1 and +-(1 - 1e-7): the clamp of normalize_inv.  The clamp is
    that of the dtype (torch's SigmoidTransform), so an f32 and an f64 evaluation of these rows differ by design."""
    obs = draw(m, 8, seed=78)
    vals = torch.tensor([1.0, -1.0, 1.0 - 1e-7, -(1.0 - 1e-7)])
    obs["thickness"][:4, 0] = vals
    obs["intensity"][4:8, 0] = vals
    return obs


def outside_rows(m, n=5):
    """`n` rows whose spline input lies outside the bound in every row: the spline's parameters must get exactly zero."""
    sp, mech = spline_of(m), spline_var(m)
    obs = draw(m, n, seed=79)
    obs[mech.var][:, 0] = torch.linspace(float(sp.bound) + 0.25, float(sp.bound) + 4.0, n) * torch.tensor([1.0, -1.0] * n)[:n]
    return obs


def knot_rows(m):
    """One observation per interior knot of the spline's image: the f32 module's own knot value (for a normalised variable the
    observation whose normalize_inv is the knot, up to rounding).  Returns a list of single-row batches."""
    from causal_gen_amd.pgm import normalize_fwd

    sp, mech = spline_of(m), spline_var(m)
    if sp is None:
        return []
    with torch.no_grad():
        yk = sp._knots()[1][0, 1:-1].clone()
    base = draw(m, len(yk), seed=77)
    rows = []
    for i, y in enumerate(yk):
        o = {k: v[i:i + 1].clone() for k, v in base.items()}
        o[mech.var][0, 0] = normalize_fwd(y) if mech.normalize else y
        rows.append(o)
    return rows
