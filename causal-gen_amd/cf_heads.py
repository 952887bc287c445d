"""What ``cf_train.CfTrainStep`` asks of an anticausal predictor, behind one interface with two implementations: the CNN heads of
``predictor.make_predictor`` (``PredHead`` records, ``cgen_predictor_*``) and mimic's ``predictor_resnet.ChestPredictor``
(``ResnetArgs``, ``cgen_resnet_*``).

A seam names the variables (``scored``: one loss term per sample each; ``ctx``: context variables the heads need as dense
``[B, k]`` buffers; ``every``: all it reads, in first-use order), builds its records once per static batch from ``at(var)`` =
(device address, row stride in floats) and ``dense[var]``, and launches on them: ``forward`` on ``cf_x`` writes ``terms``
``[B, n_terms]`` and the summed ``loss``, ``backward`` writes ``dx = coef d loss / d cf_x`` with the device coefficient ``coef``
(``1 / B``), ``scalar_nll`` is the addend of the heads that see no image (``None`` without any), ``replayed`` is called after a
captured step was replayed (the host-side notes a forward leaves, which a replay does not run).  Nothing here reads the device.
"""
import math

import torch

from . import _lib


class CnnHeads:
    """The CNN heads: today's launches of the step, one for one (``predictor._route / _fwd / _bwd`` on caller-owned buffers)."""

    def __init__(self, pred, device):
        self.pred, self.device, self.lib = pred, device, _lib.require_gpu()
        heads = pred._heads()
        self.scored = [hd.var for hd in heads]
        self.ctx = list(dict.fromkeys(hd.ctx_var for hd in heads if hd.ctx_var is not None))
        extra = [v for sh in pred._scalar_heads() for v in (sh.var, *sh.inputs)]
        self.every = list(dict.fromkeys(self.scored + self.ctx + extra))
        self.n_terms = len(heads)

    def build(self, B, xshape, at, dense):
        """``predictor._records`` on caller-owned buffers, and the placement the launches take."""
        from . import predictor as P

        heads = self.pred._heads()
        recs = (_lib.PredHead * len(heads))()
        keep = []
        for r, hd in zip(recs, heads):
            y = dense[hd.ctx_var] if hd.cnn.context_dim else None
            P.fill_head(r, hd, xshape, self.pred.std_fixed, None if y is None else y.shape[1])
            wb = hd.cnn.folded(self.device)
            keep.append(wb)
            for i, (w, b) in enumerate(wb):
                r.w[i], r.b[i] = w.data_ptr(), b.data_ptr()
            if y is not None:
                r.y = y.data_ptr()
            r.obs, r.obs_stride = at(hd.var)
        return {"B": B, "recs": recs, "keep": keep, "route": P._route(self.pred, recs, B, self.device)}

    def forward(self, plan, cf_x, terms, loss):
        from . import predictor as P

        P._fwd(self.lib, plan["route"], plan["recs"], plan["B"], cf_x, terms, None, loss)

    def backward(self, plan, cf_x, coef, dx):
        from . import predictor as P

        P._bwd(self.lib, plan["route"], plan["recs"], plan["B"], cf_x, coef, dx)

    def replayed(self, plan):
        pass

    @torch.no_grad()
    def scalar_nll(self, views, B):
        """``predictor._host_nll`` of the heads that see no image, as plain tensor ops on the static columns: ``Normal.log_prob``'s
        own expression without ``torch.distributions`` (whose argument validation reads the device, which a capture refuses).
        None when the predictor has no such head."""
        total = None
        for sh in self.pred._scalar_heads():
            ctx = torch.cat([views[v].reshape(B, -1) for v in sh.inputs], dim=-1)
            loc, logscale = sh.mlp(ctx).chunk(2, dim=-1)
            if sh.tanh_loc:
                loc = torch.tanh(loc)
            scale = self.pred.f(logscale)
            y = views[sh.var].reshape(loc.shape)
            nll = (((y - loc) ** 2) / (2 * scale ** 2) + scale.log() + math.log(math.sqrt(2 * math.pi))).sum()
            total = nll if total is None else total + nll
        return None if total is None else total.reshape(1)


class ChestHeads:
    """``ChestPredictor``: one trunk, four heads, one launch each way (``ChestPredictor._plan``).  ``finding`` is read in place at
    its stride both as a scored variable and as ``encoder_a``'s context, so there is no dense context copy; no scalar heads."""

    def __init__(self, pred, device):
        from .predictor_resnet import _VARS

        self.pred, self.device = pred, device
        self.scored, self.ctx, self.every = list(_VARS), [], list(_VARS)
        self.n_terms = len(_VARS)

    def build(self, B, xshape, at, dense):
        if tuple(xshape[1:]) != (self.pred.input_channels, self.pred.input_res, self.pred.input_res):
            raise ValueError(f"ChestPredictor: built for images of {(self.pred.input_channels, self.pred.input_res, self.pred.input_res)}, "
                             f"got {tuple(xshape[1:])}")
        return {"B": B, "run": self.pred._plan(B, self.device, at)}

    def forward(self, plan, cf_x, terms, loss):
        self.pred._fwd(plan["run"], terms, None, loss, x=cf_x)

    def backward(self, plan, cf_x, coef, dx):
        self.pred._bwd(plan["run"], coef, dx)

    def scalar_nll(self, views, B):
        return None

    def replayed(self, plan):
        self.pred._ran(plan["run"])  # (what ``forward`` notes on the host: the workspace holds this record's forward now)


def kind_of(pred):
    """"chest", "cnn" or None (a predictor ``CfTrainStep`` does not serve).  No device work."""
    from .predictor_resnet import ChestPredictor

    if isinstance(pred, ChestPredictor):
        return "chest"
    heads = getattr(pred, "_heads", None)
    if not callable(heads) or not callable(getattr(pred, "_scalar_heads", None)):
        return None
    try:
        heads()
    except NotImplementedError:
        return None
    return "cnn"


def heads_for(pred, device):
    kind = kind_of(pred)
    if kind is None:
        raise ValueError(f"CfTrainStep: no predictor seam for {type(pred).__name__}")
    return (ChestHeads if kind == "chest" else CnnHeads)(pred, device)
