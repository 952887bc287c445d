"""ChestPGM's anticausal predictors (mimic) -- flow_pgm.py:568-602, 659-703 and pgm/resnet.py without pyro or torchvision.

``encoder_s / encoder_r / encoder_f / encoder_a`` are four ``ResNet18`` wrappers around ONE shared GroupNorm ResNet-18 trunk
(7x7/s2 stem, GroupNorm, ReLU, MaxPool2d(3, 2, 1), four stages of two ``CustomBlock``s, spatial mean), each with its own
``Linear`` on the pooled features; ``encoder_a`` also sees ``finding``.  The reference runs the trunk once per head; here it runs
ONCE per call and feeds the four heads -- same numbers, a quarter of the work (csrc/predictor_resnet.inc, ``cgen_resnet_*``).
The predictor is frozen and in eval mode (Dropout is the identity): forward, likelihoods, ``predict`` and the input gradient
``d aux / d cf_x``.  Training these heads is ``predictor_resnet_train.ChestPredictorTrainStep``'s business, which works on this
module's parameters from outside: ``train()`` here still leaves eval mode on and ``_heads()`` still raises.

The modules are parameter holders with the reference's names, so that the 248 ``encoder_*`` keys of a reference checkpoint load
strictly; ``torch_outputs`` is the same network in plain torch ops on those parameters (any device, any dtype) for the CPU tests
and the benchmark's eager baseline -- the product path never takes it.
"""
import ctypes
from typing import Dict, List

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from . import _lib
from .predictor import _AnticausalPredictor, _cached, _col, _prep_x

_WIDTHS = (64, 128, 256, 512)
_VARS = ("sex", "race", "finding", "age")  # the order of the kernel's terms / outs
_NOUT = (1, 3, 1, 2)
MIN_RES, MAX_RES = 32, 256


def _ceil(a, m):
    return (a + m - 1) // m * m


def _norm(c):
    return nn.GroupNorm(min(32, c // 4), c)


class _Block(nn.Module):
    """resnet.py CustomBlock's parameters: conv1, bn1, conv2, bn2 and, on the first block of stages 2-4, downsample.0 / .1."""

    def __init__(self, cin, c, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, c, 3, stride, 1, bias=False)
        self.bn1 = _norm(c)
        self.conv2 = nn.Conv2d(c, c, 3, 1, 1, bias=False)
        self.bn2 = _norm(c)
        self.downsample = nn.Sequential(nn.Conv2d(cin, c, 1, stride, bias=False), _norm(c)) if stride != 1 or cin != c else None
        self.stride = stride


def _trunk(in_channels):
    """``nn.Sequential(*children[:-1])`` of the reference's ResNet: indices 0 stem, 1 norm, 2 ReLU, 3 max pool, 4-7 stages, 8 pool."""
    stages, cin = [], 64
    for s, c in enumerate(_WIDTHS):
        stages.append(nn.Sequential(_Block(cin, c, 1 if s == 0 else 2), _Block(c, c, 1)))
        cin = c
    return nn.Sequential(nn.Conv2d(in_channels, 64, 7, 2, 3, bias=False), _norm(64), nn.ReLU(), nn.MaxPool2d(3, 2, 1), *stages,
                         nn.AdaptiveAvgPool2d(1))


class ResNet18(nn.Module):
    """resnet.py ResNet18: ``resnet`` (the shared trunk) and ``fc = Linear(512 + context_dim, num_outputs)``."""

    def __init__(self, trunk, num_outputs=1, context_dim=0):
        super().__init__()
        self.num_outputs, self.context_dim = num_outputs, context_dim
        self.resnet = trunk
        self.fc = nn.Linear(512 + context_dim, num_outputs)


def _blocks(trunk) -> List[_Block]:
    return [trunk[4 + s][j] for s in range(4) for j in range(2)]


def _conv_sites(trunk):
    """[(conv, norm, runs on patches)] in the kernel's order: stem; conv1, conv2 of blocks 0..7; the identity convs of stages 2-4."""
    sites = [(trunk[0], trunk[1], True)]
    for b in _blocks(trunk):
        sites += [(b.conv1, b.bn1, b.stride != 1), (b.conv2, b.bn2, False)]
    sites += [(trunk[4 + s][0].downsample[0], trunk[4 + s][0].downsample[1], False) for s in (1, 2, 3)]
    return sites


class _ChestNLL(torch.autograd.Function):
    """sum over samples and the four heads of -log q(parent | x, ...): one forward plan, one backward plan."""

    @staticmethod
    def forward(ctx, x, owner, obs):
        xd = _prep_x(x)
        run = owner._run(xd, obs, need_obs=True)
        terms = torch.empty(xd.shape[0], 4, device=xd.device)
        loss = torch.empty(1, device=xd.device)
        owner._fwd(run, terms, None, loss)
        ctx.state = (owner, run, obs, x.device, x.dtype)
        return loss[0].to(x.device)

    @staticmethod
    def backward(ctx, g):
        owner, run, obs, xdev, xdt = ctx.state
        if owner.__dict__.get("_ws_token") is not run["token"]:  # another call has used the workspace since: run the forward again
            run = owner._run(run["x"], obs, need_obs=True)
            owner._fwd(run, torch.empty(run["n"], 4, device=run["x"].device), None, None)
        coef = g.detach().reshape(1).float().to(run["x"].device).contiguous()
        dx = torch.empty_like(run["x"])
        owner._bwd(run, coef, dx)
        return dx.to(device=xdev, dtype=xdt), None, None


class ChestPredictor(_AnticausalPredictor):
    """flow_pgm.py:568-602, 659-703 (mimic): q(s | x), q(f | x) Bernoulli(sigmoid); q(r | x) OneHotCategorical(softmax);
    q(a | x, f) Normal(loc, f(logscale)) -- no tanh.  ``input_channels`` 1, square ``input_res`` 32..256 (odd sizes too), B >= 1."""

    def __init__(self, args):
        super().__init__(args)
        self.input_channels, self.input_res = int(args.input_channels), int(args.input_res)
        trunk = _trunk(self.input_channels)
        self.encoder_s = ResNet18(trunk, num_outputs=1)
        self.encoder_r = ResNet18(trunk, num_outputs=3)
        self.encoder_f = ResNet18(trunk, num_outputs=1)
        self.encoder_a = ResNet18(trunk, num_outputs=2, context_dim=1)
        self.eval()

    def _encoders(self):
        return [self.encoder_s, self.encoder_r, self.encoder_f, self.encoder_a]

    def load_reference_state_dict(self, sd: Dict[str, Tensor]):
        """As the other predictors; the four trunk copies of a reference checkpoint hold equal values and land in the one trunk."""
        kept = {k: v for k, v in sd.items() if k.split(".")[0].startswith("encoder_")}
        for k, v in kept.items():
            head, rest = k.split(".", 1)
            if rest.startswith("resnet.") and head != "encoder_s":
                first = kept.get("encoder_s." + rest)
                if first is not None and not torch.equal(first, v):
                    raise ValueError(f"load_reference_state_dict: {k} differs from encoder_s.{rest}: the heads share one trunk here")
        dropped = sorted(set(sd) - set(kept))
        self.load_state_dict(kept, strict=True)
        return dropped

    # ------------------------------------------------------------------ plain torch (CPU tests, the benchmark's eager baseline)
    @staticmethod
    def _gn(x, m):
        return F.group_norm(x, m.num_groups, m.weight.to(x.dtype), m.bias.to(x.dtype), m.eps)

    def torch_features(self, x: Tensor) -> Tensor:
        """The pooled trunk features [B, 512] in plain torch ops on the module's own parameters, in ``x``'s dtype."""
        t = self.encoder_s.resnet
        cv = lambda h, m: F.conv2d(h, m.weight.to(h.dtype), None, m.stride, m.padding)
        h = F.max_pool2d(F.relu(self._gn(cv(x, t[0]), t[1])), 3, 2, 1)
        for b in _blocks(t):
            idn = h if b.downsample is None else self._gn(cv(h, b.downsample[0]), b.downsample[1])
            o = F.relu(self._gn(cv(h, b.conv1), b.bn1))
            h = F.relu(self._gn(cv(o, b.conv2), b.bn2) + idn)
        return h.mean(dim=(2, 3))

    def torch_outputs(self, x: Tensor, finding: Tensor, shared: bool = True) -> Dict[str, Tensor]:
        """{variable: [B, nout]} raw head outputs in plain torch; ``shared=False`` runs the trunk once per head as the reference does."""
        B = x.shape[0]
        out, feat = {}, None
        for var, enc in zip(_VARS, self._encoders()):
            if feat is None or not shared:
                feat = self.torch_features(x)
            f = feat if not enc.context_dim else torch.cat([feat, finding.reshape(B, -1).to(feat.dtype)], dim=-1)
            out[var] = F.linear(f, enc.fc.weight.to(f.dtype), enc.fc.bias.to(f.dtype))
        return out

    # ------------------------------------------------------------------ device state
    def _state_key(self, device):
        ps = list(self.parameters())
        return (str(device),) + tuple(p._version for p in ps) + tuple(p.data_ptr() for p in ps)

    @torch.no_grad()
    def _weight_tables(self, device):
        """The 40 weight images (cgen_weight_prep modes 0 / 1, f32; empty) and the launch's descriptor and chunk tables on
        ``device``.  ``srcs`` are the f32 parameters the descriptors read: the parameters themselves where they already are
        contiguous f32 tensors on ``device``."""
        dev32 = lambda t: t.detach().to(device=device, dtype=torch.float32).contiguous()
        sites = _conv_sites(self.encoder_s.resnet)
        descs, srcs, fwd, dg = [], [], [], []
        for conv, _, patches in sites:
            w = dev32(conv.weight)
            srcs.append(w)
            co, ci, ks = w.shape[0], w.shape[1], w.shape[2]
            if patches:  # the conv runs as a 1x1 conv on a patch tensor: the OIHW parameter is its [co][ci * ks * ks] matrix
                ci, ks = ci * ks * ks, 1
            taps = ks * ks
            krow, krow_dg = _ceil(taps * _ceil(ci, 8), 32) + 32, _ceil(taps * _ceil(co, 8), 32) + 32
            for mode, rows, k in ((0, _ceil(co, 16), krow), (1, _ceil(ci, 16), krow_dg)):
                img = torch.empty(rows * k, dtype=torch.float32, device=device)
                d = _lib.WprepDesc()
                d.src, d.dst = w.data_ptr(), img.data_ptr()
                d.co, d.ci_total, d.ks, d.mode, d.nseg, d.seg_off = co, ci, ks, mode, 1, 0
                d.seg_c[0] = ci
                d.dtype, d.rows_pad, d.k_pad, d.numel = _lib.F32, rows, k, rows * k
                descs.append(d)
                (fwd if mode == 0 else dg).append(img)
        chunk = 1024  # elements per workgroup of cgen_weight_prep
        csite, cidx = [], []
        for i, d in enumerate(descs):
            nch = (d.numel + chunk - 1) // chunk
            csite += [i] * nch
            cidx += list(range(nch))
        tab = torch.frombuffer(bytearray(bytes((_lib.WprepDesc * len(descs))(*descs))), dtype=torch.uint8).to(device)
        cs, ci_ = (torch.tensor(v, dtype=torch.int32, device=device) for v in (csite, cidx))
        return {"fwd": fwd, "dg": dg, "srcs": srcs, "tab": tab, "csite": cs, "cidx": ci_, "nchunks": len(csite)}

    @torch.no_grad()
    def _images(self, device):
        """The weight images (cgen_weight_prep modes 0 / 1, f32), GroupNorm parameters and head weights on ``device``; rebuilt
        when a parameter's version or address changes."""
        key = self._state_key(device)
        rt = self.__dict__.get("_rt")
        if rt is not None and rt[0] == key:
            return rt[1]
        lib = _lib.require_gpu()
        dev32 = lambda t: t.detach().to(device=device, dtype=torch.float32).contiguous()
        sites = _conv_sites(self.encoder_s.resnet)
        wt = self._weight_tables(device)
        lib.weight_prep(wt["tab"].data_ptr(), wt["csite"].data_ptr(), wt["cidx"].data_ptr(), wt["nchunks"],
                        torch.cuda.current_stream(device).cuda_stream)
        out = {"fwd": wt["fwd"], "dg": wt["dg"], "gamma": [dev32(n.weight) for _, n, _ in sites], "beta": [dev32(n.bias) for _, n, _ in sites],
               "fc_w": [dev32(e.fc.weight) for e in self._encoders()], "fc_b": [dev32(e.fc.bias) for e in self._encoders()]}
        self.__dict__["_rt"] = (key, out)
        return out

    def _check(self, x: Tensor):
        if x.dim() != 4 or x.shape[0] < 1 or x.shape[1] != 1 or self.input_channels != 1:
            raise ValueError(f"ChestPredictor: needs x of [B >= 1, 1, R, R] and input_channels 1, got {tuple(x.shape)} "
                             f"(input_channels {self.input_channels})")
        R = x.shape[-1]
        if x.shape[-2] != R or R != self.input_res or not MIN_RES <= R <= MAX_RES:
            raise ValueError(f"ChestPredictor: built for square images of input_res {self.input_res} within {MIN_RES}..{MAX_RES}, "
                             f"got {tuple(x.shape[-2:])}")

    def _net_args(self, dev, R):
        """(the argument record with the network's side filled in -- weight images, GroupNorm parameters, heads --, what it points into)"""
        im = self._images(dev)
        a = _lib.ResnetArgs()
        a.res, a.std_fixed = R, self.std_fixed
        for i in range(_lib.RESNET_CONVS):
            a.img_fwd[i], a.img_dg[i] = im["fwd"][i].data_ptr(), im["dg"][i].data_ptr()
            a.gamma[i], a.beta[i] = im["gamma"][i].data_ptr(), im["beta"][i].data_ptr()
        for h in range(4):
            a.fc_w[h], a.fc_b[h] = im["fc_w"][h].data_ptr(), im["fc_b"][h].data_ptr()
        return a, im

    def _plan(self, n: int, dev, at):
        """``_run``'s record on caller-owned buffers: ``at(var)`` = (device address, row stride in floats) of a variable's rows --
        a static buffer, or a column of a wider table (``race``: three adjacent columns from that address; ``finding`` is both the
        scored variable and ``encoder_a``'s context, read in place at its stride).  Nothing is copied, so a captured launch sees
        whatever the buffers hold when it replays.  The image is not part of the record: ``_fwd(run, ..., x=...)`` binds it at
        launch time and ``_bwd`` reads the workspace.  The record holds its workspace: a later, larger call may give the
        predictor another one, this one stays allocated for as long as the record (and a graph captured over it) lives."""
        lib = _lib.require_gpu()
        dev = torch.device(dev)
        if dev.index is None:  # (the cached weight images and workspace are keyed by the device as tensors name it)
            dev = torch.device(dev.type, torch.cuda.current_device())
        n, R = int(n), self.input_res
        if n < 1 or self.input_channels != 1 or not MIN_RES <= R <= MAX_RES:
            raise ValueError(f"ChestPredictor: needs B >= 1, input_channels 1 and input_res within {MIN_RES}..{MAX_RES}, got B = {n}, "
                             f"input_channels {self.input_channels}, input_res {R}")
        a, im = self._net_args(dev, R)
        for h, var in enumerate(_VARS):
            ptr, stride = at(var)
            if not ptr or int(stride) < (3 if var == "race" else 1):
                raise ValueError(f"ChestPredictor: {var!r} at address {ptr} with a row stride of {stride} floats")
            a.obs[h], a.obs_stride[h] = int(ptr), int(stride)
            if var == "finding":
                a.ctx, a.ctx_stride = int(ptr), int(stride)
        need = _lib.i64(0)
        lib.resnet_workspace(n, R, ctypes.byref(need))
        ws = _cached(self, "_ws", need.value, dev)
        return {"lib": lib, "args": a, "keep": [im], "ws": ws, "n": n, "res": R, "x": None, "token": object()}

    def _run(self, x: Tensor, obs, need_obs: bool):
        """Everything a launch plan needs: the argument record, the tensors it points into, the workspace."""
        self._check(x)
        lib = _lib.require_gpu()
        dev, B, R = x.device, x.shape[0], x.shape[-1]
        a, im = self._net_args(dev, R)
        keep = [im]
        if "finding" not in obs:
            raise ValueError("ChestPredictor: the age head needs obs['finding']")
        fnd = _col(obs["finding"], B, dev)
        keep.append(fnd)
        a.ctx, a.ctx_stride = fnd.data_ptr(), fnd.shape[1]
        if need_obs:
            for h, var in enumerate(_VARS):
                o = fnd if var == "finding" else _col(obs[var], B, dev)
                if o.shape[1] < (3 if var == "race" else 1):
                    raise ValueError(f"ChestPredictor: obs[{var!r}] has {o.shape[1]} columns")
                keep.append(o)
                a.obs[h], a.obs_stride[h] = o.data_ptr(), o.shape[1]
        need = _lib.i64(0)
        lib.resnet_workspace(B, R, ctypes.byref(need))
        ws = _cached(self, "_ws", need.value, dev)
        return {"lib": lib, "args": a, "keep": keep, "ws": ws, "n": B, "res": R, "x": x, "token": object()}

    def _ran(self, run):
        """Host-side note that `run`'s forward is the last one enqueued: ``_fwd`` leaves it, and so does whoever replays a graph
        captured over ``_fwd`` (a replay runs no Python).  ``_ChestNLL.backward`` reads the token (its forward's state may be gone),
        ``trunk_activations`` the shape and the record's workspace, whatever ``_ws`` is by now."""
        self.__dict__["_ws_token"] = run["token"]
        self.__dict__["_ws_shape"] = (run["n"], run["res"])
        self.__dict__["_ws_last"] = run["ws"]

    def _fwd(self, run, terms, outs, loss, x: Tensor = None):
        """The forward launch of a record; `x` (a contiguous f32 device image batch) for a record of ``_plan``, which holds none."""
        t, o, l = (v.data_ptr() if v is not None else None for v in (terms, outs, loss))
        ws = run["ws"]
        if x is None:
            x = run["x"]
        else:
            self._check(x)
            if x.shape[0] != run["n"] or x.dtype != torch.float32 or not x.is_contiguous() or x.device != ws.device:
                raise ValueError(f"ChestPredictor: the plan was built for {run['n']} contiguous f32 images on {ws.device}")
        self._ran(run)
        run["lib"].resnet_fwd(ctypes.byref(run["args"]), run["n"], x.data_ptr(), ws.data_ptr(), ws.numel(), t, o, l,
                              torch.cuda.current_stream(x.device).cuda_stream)

    def _bwd(self, run, coef, dx):
        ws = run["ws"]
        run["lib"].resnet_bwd(ctypes.byref(run["args"]), run["n"], ws.data_ptr(), ws.numel(), coef.data_ptr(), dx.data_ptr(),
                              torch.cuda.current_stream(dx.device).cuda_stream)

    # ------------------------------------------------------------------ the predictors' surface
    def _heads(self):
        # (no CNN head records: the ResNet heads have an entry point of their own, and only the CNN training step asks for these)
        raise NotImplementedError("ChestPredictor: training mimic's ResNet-18 heads (PredictorTrainStep) is not implemented; "
                                  "this predictor is the frozen, eval-mode one")

    def path(self, x: Tensor) -> str:
        return "resnet"

    def model_anticausal(self, **obs) -> Tensor:
        aux = {k: v for k, v in obs.items() if k != "x" and isinstance(v, Tensor)}
        return _ChestNLL.apply(obs["x"], self, aux)

    @torch.no_grad()
    def nll_terms(self, **obs) -> Dict[str, Tensor]:
        x = _prep_x(obs["x"])
        run = self._run(x, obs, need_obs=True)
        terms = torch.empty(x.shape[0], 4, device=x.device)
        self._fwd(run, terms, None, None)
        return {var: terms[:, h] for h, var in enumerate(_VARS)}

    def _outputs(self, obs) -> Dict[str, Tensor]:
        x = _prep_x(obs["x"])
        run = self._run(x, obs, need_obs=False)
        outs = torch.empty(4, x.shape[0], _lib.PRED_MAX_OUT, device=x.device)
        self._fwd(run, None, outs, None)
        return {var: outs[h, :, :_NOUT[h]] for h, var in enumerate(_VARS)}

    @torch.no_grad()
    def predict(self, **obs) -> Dict[str, Tensor]:
        o = self._outputs(obs)
        return {"sex": torch.sigmoid(o["sex"]), "race": F.softmax(o["race"], dim=-1), "finding": torch.sigmoid(o["finding"]),
                "age": o["age"][:, :1]}

    @torch.no_grad()
    def trunk_activations(self, x: Tensor = None) -> List[Tensor]:
        """f32 NCHW copies, on the device, of what the last forward left in its workspace: the 17 post-ReLU activations in order
        (the stem, then relu(bn1) and the block output of each of the eight blocks) and, last, the max-pool's output.  With ``x``
        a forward on it (``finding`` = 0: the trunk does not see it) runs first."""
        if x is not None:
            self._outputs({"x": x, "finding": torch.zeros(x.shape[0], 1)})
        ws, shape = self.__dict__.get("_ws_last"), self.__dict__.get("_ws_shape")
        if ws is None or shape is None:
            raise RuntimeError("ChestPredictor.trunk_activations: no forward has run yet")
        lib = _lib.load()
        n, res = shape
        out = []
        for site in range(_lib.RESNET_SITES):
            off, h, c = _lib.i64(0), _lib.i32(0), _lib.i32(0)
            lib.resnet_site(n, res, site, ctypes.byref(off), ctypes.byref(h), ctypes.byref(c))
            v = ws[off.value:off.value + n * h.value * h.value * c.value].view(n, h.value, h.value, c.value)
            out.append(v.permute(0, 3, 1, 2).contiguous())
        return out

    def __deepcopy__(self, memo):
        import copy as _copy

        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k not in ("_ws", "_ws_last", "_ws_token", "_ws_shape", "_rt"):  # runtime workspaces and weight images: rebuilt on first use
                new.__dict__[k] = _copy.deepcopy(v, memo)
        return new
