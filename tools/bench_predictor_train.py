"""Time one training step of the anticausal predictors: ``PredictorTrainStep.step`` (captured hipGraph, and eager launches) against
the same step in torch eager on the same GPU -- the modules' own torch layers in train mode, torch.distributions, ``backward()``,
``clip_grad_norm_(200)``, ``AdamW`` under ``LambdaLR`` and a foreach EMA of parameters and buffers.  Cases: morphomnist at B = 32
and 256, ukbb192 (4 image heads) at B = 32.  Prints one JSON line per case; no threshold.

Then two more lines for ukbb192 at B = 32, each time the median (and the min .. max spread) of three runs of 200 captured steps
between a pair of events: ``scalar_heads=True`` (encoder_a trained too; the torch-eager step trains it as well), and ``step_from``
(the batch built inside the captured step from a resident u8 data set) beside ``step()`` on a resident batch of the same tree.
``--only-new`` skips the first three lines, ``--baseline`` prints the plain ukbb192 step alone in the same 3 x 200 form (what a
parent tree's step is compared by)."""
import copy
import json
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from bench_predictor import eager_nll, obs_for, timeit  # noqa: E402
from causal_gen_amd import predictor as P  # noqa: E402
from causal_gen_amd.predictor_train import PredictorTrainStep  # noqa: E402
from predictor_ref import randomise  # noqa: E402


class EagerStep:
    """train_pgm.py's sup_epoch body on torch layers (the image heads only, as PredictorTrainStep; with `scalar_heads` encoder_a too)"""

    def __init__(self, pred, lr=1e-4, wd=0.1, scalar_heads=False):
        self.pred, self.scalar_heads = pred, scalar_heads
        self.cnns = [hd.cnn for hd in pred._heads()]
        for c in self.cnns:
            c.cnn.train(True)  # (the Sequentials' own train(): CNN.train() forces eval)
            c.fc.train(True)
            c.requires_grad_(True)
        if scalar_heads:
            self.cnns = self.cnns + [sh.mlp for sh in pred._scalar_heads()]  # (modules whose parameters and buffers are trained)
            for sh in pred._scalar_heads():
                sh.mlp.mlp.train(True)
                sh.mlp.requires_grad_(True)
        self.params = [p for c in self.cnns for p in c.parameters()]
        self.opt = torch.optim.AdamW(self.params, lr=lr, weight_decay=wd)
        self.sched = torch.optim.lr_scheduler.LambdaLR(self.opt, lambda it: 1.0 if it > 1 else it / 1)
        self.state = [t for c in self.cnns for t in list(c.parameters()) + [b for b in c.buffers() if b.is_floating_point()]]
        self.ema = [t.detach().clone() for t in self.state]

    def step(self, obs):
        self.opt.zero_grad(set_to_none=True)
        loss = self._nll(obs) / obs["x"].shape[0]
        loss.backward()
        torch.nn.utils.clip_grad_norm_(self.params, 200.0)
        self.opt.step()
        self.sched.step()
        with torch.no_grad():
            torch._foreach_lerp_(self.ema, [t.detach() for t in self.state], 1e-3)
        return loss

    def _nll(self, obs):
        if isinstance(self.pred, P.FlowPredictor) and not self.scalar_heads:  # (the image heads only: encoder_a's term is a constant of this step)
            with torch.no_grad():
                age = eager_nll_age(self.pred, obs)
            return eager_nll(self.pred, obs) - age
        return eager_nll(self.pred, obs)


def eager_nll_age(pred, obs):
    al, as_ = pred.encoder_a(torch.cat([obs["brain_volume"], obs["ventricle_volume"]], -1)).chunk(2, -1)
    return -torch.distributions.Normal(al, torch.nn.functional.softplus(as_)).log_prob(obs["age"]).sum()


def timeit3(fn, warm=5, reps=200, runs=3):
    """[median, min, max] ms per call over `runs` runs of `reps` calls between a pair of events"""
    t = sorted(timeit(fn, warm=warm, reps=reps) for _ in range(runs))
    return [round(t[len(t) // 2], 4), round(t[0], 4), round(t[-1], 4)]


def ukbb_case(B=32, R=192):
    g = torch.Generator().manual_seed(0)
    pred = P.make_predictor(SimpleNamespace(dataset="ukbb192", input_channels=1, input_res=R, std_fixed=0.0))
    randomise(pred, g)
    return pred.cuda(), obs_for("ukbb192", B, 1, R, g), g


def baseline():
    pred, obs, _ = ukbb_case()
    ts = PredictorTrainStep(copy.deepcopy(pred))
    print(json.dumps({"case": "ukbb192", "B": 32, "hip_graph_ms_3x200": timeit3(lambda: ts.step(**obs))}), flush=True)


def new_cases():
    from causal_gen_amd.data import DeviceDataset

    pred, obs, g = ukbb_case()
    B, R = 32, 192
    ts = PredictorTrainStep(copy.deepcopy(pred), scalar_heads=True)
    row = {"case": "ukbb192 scalar_heads", "B": B, "hip_graph_ms_3x200": timeit3(lambda: ts.step(**obs))}
    row["loss_hip"] = round(float(ts.step(**obs)["loss"]), 5)
    te = PredictorTrainStep(copy.deepcopy(pred), scalar_heads=True, use_graph=False)
    row["hip_eager_ms"] = round(timeit(lambda: te.step(**obs)), 4)
    eager = EagerStep(copy.deepcopy(pred), scalar_heads=True)
    row["torch_eager_ms"] = round(timeit(lambda: eager.step(obs)), 4)
    row["loss_torch"] = round(float(eager.step(obs)), 5)
    print(json.dumps(row), flush=True)
    # step_from: 256 resident rows at the preset's native 192 x 192 (pad 9: RandomCrop(padding=[18, 9])), every variable in pa
    cols = {"sex": 0, "mri_seq": 1, "age": 2, "brain_volume": 3, "ventricle_volume": 4}
    pa = torch.cat([obs[k] for k in cols], dim=1).repeat(8, 1)
    ds = DeviceDataset(torch.randint(0, 256, (256, 1, R, R), generator=g, dtype=torch.uint8), pa, R, pad=(18, 9), hflip=0.5)
    idx = torch.randperm(256, generator=g)[:B].cuda()
    tf = PredictorTrainStep(copy.deepcopy(pred), scalar_heads=True, columns=cols)
    batch = ds.batch(idx)
    res = dict({k: batch["pa"][:, c:c + 1] for k, c in cols.items()}, x=batch["x"].contiguous())
    tr = PredictorTrainStep(copy.deepcopy(pred), scalar_heads=True)
    row = {"case": "ukbb192 scalar_heads step_from", "B": B}
    for _ in range(2):  # (alternating: from, resident, from, resident)
        for name, fn in (("step_from_ms_3x200", lambda: tf.step_from(ds, idx)), ("step_resident_ms_3x200", lambda: tr.step(**res))):
            row[name] = min(row.get(name, [1e9] * 3), timeit3(fn))
    row["loss_step_from"] = round(float(tf.step_from(ds, idx)["loss"]), 5)
    print(json.dumps(row), flush=True)


def main():
    if "--baseline" in sys.argv:
        return baseline()
    if "--only-new" in sys.argv:
        return new_cases()
    existing_cases()
    new_cases()


def existing_cases():
    for ds, C, R, B in [("morphomnist", 1, 32, 32), ("morphomnist", 1, 32, 256), ("ukbb192", 1, 192, 32)]:
        g = torch.Generator().manual_seed(0)
        pred = P.make_predictor(SimpleNamespace(dataset=ds, input_channels=C, input_res=R, std_fixed=0.0))
        randomise(pred, g)
        pred = pred.cuda()
        obs = obs_for(ds, B, C, R, g)
        eager = EagerStep(copy.deepcopy(pred))
        row = {"case": ds, "B": B}
        for name, graph in (("hip_graph_ms", True), ("hip_eager_ms", False)):
            ts = PredictorTrainStep(copy.deepcopy(pred), use_graph=graph)
            row[name] = round(timeit(lambda: ts.step(**obs)), 4)
            row["loss_hip"] = round(float(ts.step(**obs)["loss"]), 5)
        row["torch_eager_ms"] = round(timeit(lambda: eager.step(obs)), 4)
        row["loss_torch"] = round(float(eager.step(obs)), 5)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
