"""The smallest mimic fixture for ``CfTrainStep`` with a ``ChestPredictor``: the recipe of ``chest_dscm`` in
tests/test_gpu_predictor_resnet.py (a mimic192 HVAE shrunk to 32 x 32 pixels, ``ChestPGM``, the randomised GroupNorm ResNet-18 heads)
built on the CPU; the GPU tests move its parts to the device.  R = 32 is ``ChestPredictor``'s minimum, B = 3 is odd and no multiple
of any tile, B = 2 is the second batch shape.  The data set of ``step_from``: 8 u8 rows of [1, 32, 32] and the [8, 6] parents table
of ``scm.sample(8)`` in ``default_columns`` order (race 0-2, sex 3, finding 4, age 5); mimic has no augmentation."""
from types import SimpleNamespace

import torch

import pgm_cases as PC
from resnet_ref import randomise

LMBDA0, EPS_C, DAMPING = 1.0, 2.0, 10.0
LR, LR_LAG = 1e-3, 1e-2
# w = lmbda - damping (eps - elbo) multiplies the ELBO's gradient: the preset's own threshold of 500 would drop the steps.  Every test
# that compares steps taken asserts n_skipped == 0 next to it.
GRAD_SKIP = 1e5  # (the f64 oracle's gradient norm on this fixture is 157)
VARS = ("sex", "race", "finding", "age")
COLUMNS = {"race": 0, "sex": 3, "finding": 4, "age": 5}
WIDTH = {"race": 3, "sex": 1, "finding": 1, "age": 1}
N_DATA = 8


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def hparams(**over):
    from causal_gen_amd.hps import setup_hparams

    hp = setup_hparams("mimic192", input_res=32, enc_arch="32b1d2,16b1d2,8b1d8,1b1", dec_arch="1b1,8b1,16b1,32b1", widths=[16, 32, 48, 64],
                       z_max_res=16, pad=0)
    hp.dataset = "mimic"
    hp.lmbda_init, hp.elbo_constraint, hp.damping, hp.std_fixed = LMBDA0, EPS_C, DAMPING, 0.0
    hp.grad_skip = GRAD_SKIP
    for k, v in over.items():
        setattr(hp, k, v)
    return hp


def parts(B=3, **over):
    """(hp, HVAE, ChestPGM, ChestPredictor, parents {variable: [B, k]}, x [B, 1, 32, 32]) on the CPU, f32."""
    from causal_gen_amd import vae
    from causal_gen_amd.predictor_resnet import ChestPredictor
    from oracle import fullsize_recipe as FR

    hp = hparams(**over)
    torch.manual_seed(7)
    m = vae.HVAE(hp)
    m.apply(FR.init_bias)
    FR.perturb(m)
    m.compute_dtype = "f32"
    m.eval()
    scm = PC.make_pgm("chest", seed=0)
    pred = randomise(ChestPredictor(hp), 11)
    g = torch.Generator().manual_seed(3)
    pa = scm.sample(B, torch.Generator().manual_seed(5))
    x = (torch.randint(0, 256, (B, 1, 32, 32), generator=g).float() - 127.5) / 127.5
    return hp, m, scm, pred, pa, x


def cf_of(pa):
    """Fixed counterfactual values of the four variables: sex and finding flipped, race rolled one class on, age moved."""
    return {"sex": 1.0 - pa["sex"], "race": pa["race"].roll(1, 1), "finding": 1.0 - pa["finding"], "age": 0.5 * pa["age"] + 0.25}


def compact(hp, pa):
    """[B, 6] parents in ``args.parents_x`` order (what ``vae_preprocess`` concatenates, before its expansion)."""
    return torch.cat([pa[k].reshape(pa[k].shape[0], -1) for k in hp.parents_x], 1).float()


class FixedPGM(torch.nn.Module):
    """``pgm.counterfactual`` of the host composition with a fixed answer."""

    def __init__(self, cf):
        super().__init__()
        self.cf = cf

    def counterfactual(self, obs, intervention, num_particles=1):
        return {k: v.cuda() for k, v in self.cf.items()}


def make(B=3, use_graph=False, ema=True, pgm="fixed", **over):
    """SimpleNamespace(hp, model (DSCM on the device), step, x, pa, cf (the fixed counterfactual variables), pa_c / cf_c (compact
    parents), scm, pred), all tensors on the device.  ``pgm="scm"`` hands the DSCM the ChestPGM itself (``step_from``)."""
    from causal_gen_amd import dscm
    from causal_gen_amd.cf_train import CfTrainStep

    hp, m, scm, pred, pa, x = parts(B, **over)
    cf = cf_of(pa)
    model = dscm.DSCM(hp, FixedPGM(cf) if pgm == "fixed" else scm, pred, m).cuda()
    for p in m.parameters():
        p.requires_grad_(True)
    step = CfTrainStep(model, hp, lr=LR, lr_lagrange=LR_LAG, ema=ema, use_graph=use_graph)
    dev = lambda d: {k: v.cuda() for k, v in d.items()}  # noqa: E731
    return SimpleNamespace(hp=hp, model=model, step=step, x=x.cuda(), pa=dev(pa), cf=dev(cf), pa_c=compact(hp, pa).cuda(),
                           cf_c=compact(hp, cf).cuda(), scm=model.pgm, pred=model.predictor, vae=model.vae)


def dataset(device="cuda"):
    """(DeviceDataset of 8 u8 images without crop or flip freedom, the [8, 6] parents table on the CPU)"""
    from causal_gen_amd.data import DeviceDataset

    scm = PC.make_pgm("chest", seed=0)
    obs = scm.sample(N_DATA, torch.Generator().manual_seed(41))
    table = torch.zeros(N_DATA, 6)
    for var, c0 in COLUMNS.items():
        table[:, c0:c0 + WIDTH[var]] = obs[var]
    x_u8 = torch.randint(0, 256, (N_DATA, 1, 32, 32), generator=torch.Generator().manual_seed(21), dtype=torch.uint8)
    return DeviceDataset(x_u8, table, 32, pad=(0, 0), hflip=0.0, device=device), table


def snapshot(model, step):
    torch.cuda.synchronize()
    return {"w": {k: v.clone() for k, v in model.vae.state_dict().items()}, "ema": {k: v.clone() for k, v in step.ema_vae.state_dict().items()},
            "lag": step.lag.clone(), "m": step.tail.m.clone(), "v": step.tail.v.clone(), "res": step.res.clone(), "sums": step.sums.clone()}


def same(a, b, skip=()):
    for k in ("lag", "m", "v", "res", "sums"):
        if k not in skip:
            assert torch.equal(bits(a[k]), bits(b[k])), k
    for part in ("w", "ema"):
        for k in a[part]:
            assert torch.equal(a[part][k], b[part][k]), (part, k)
