"""Time one training step of the anticausal predictors: ``PredictorTrainStep.step`` (captured hipGraph, and eager launches) against
the same step in torch eager on the same GPU -- the modules' own torch layers in train mode, torch.distributions, ``backward()``,
``clip_grad_norm_(200)``, ``AdamW`` under ``LambdaLR`` and a foreach EMA of parameters and buffers.  Cases: morphomnist at B = 32
and 256, ukbb192 (4 image heads) at B = 32.  Prints one JSON line per case; no threshold."""
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
    """train_pgm.py's sup_epoch body on torch layers (the image heads only, as PredictorTrainStep)"""

    def __init__(self, pred, lr=1e-4, wd=0.1):
        self.pred = pred
        self.cnns = [hd.cnn for hd in pred._heads()]
        for c in self.cnns:
            c.cnn.train(True)  # (the Sequentials' own train(): CNN.train() forces eval)
            c.fc.train(True)
            c.requires_grad_(True)
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
        if isinstance(self.pred, P.FlowPredictor):  # (the image heads only: encoder_a's term is a constant of this step)
            with torch.no_grad():
                age = eager_nll_age(self.pred, obs)
            return eager_nll(self.pred, obs) - age
        return eager_nll(self.pred, obs)


def eager_nll_age(pred, obs):
    al, as_ = pred.encoder_a(torch.cat([obs["brain_volume"], obs["ventricle_volume"]], -1)).chunk(2, -1)
    return -torch.distributions.Normal(al, torch.nn.functional.softplus(as_)).log_prob(obs["age"]).sum()


def main():
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
