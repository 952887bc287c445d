"""f64 torch restatement of ChestPGM's anticausal heads for the ChestPredictor tests: the GroupNorm ResNet-18 of pgm/resnet.py
(eval mode: Dropout is the identity) read from a ``state_dict`` with the reference's key names, one Linear per head, and the
likelihoods of flow_pgm.py's model_anticausal through torch.distributions with torch's f32 clamp_probs constant.

Two modes.  Free: every ReLU and the max pool decide for themselves.  Pinned: every ReLU multiplies by a given 0/1 mask and the
max pool gathers at given indices (both taken from the activations the device computed), so that a ReLU input within rounding of
zero cannot send the two computations down different branches -- the input gradient is compared in this mode."""
import torch
import torch.nn.functional as F

EPS32 = float(torch.finfo(torch.float32).eps)
VARS = ("sex", "race", "finding", "age")
ENC = {"sex": "encoder_s", "race": "encoder_r", "finding": "encoder_f", "age": "encoder_a"}


class _MaskRelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, mask):
        ctx.save_for_backward(mask)
        return v * mask

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        return g * mask, None


def _gn(h, sd, key):
    c = h.shape[1]
    return F.group_norm(h, min(32, c // 4), sd[key + ".weight"], sd[key + ".bias"], 1e-5)


def trunk_ref(sd, x, masks=None, pool_idx=None, prefix="encoder_s.resnet."):
    """(pooled features [B, 512], acts, pres): ``acts`` = the 17 post-ReLU activations in order (stem; relu(bn1) and the output
    of each block) and, last, the max pool's output; ``pres`` = the 17 ReLU inputs.  ``masks`` (17 tensors of 0/1) and
    ``pool_idx`` ([B, 64, Hp, Wp] flat indices into the stem's map) pin the decisions."""
    dt = x.dtype
    sd = {k[len(prefix):]: v.detach().to(dtype=dt, device=x.device) for k, v in sd.items() if k.startswith(prefix)}
    acts, pres = [], []

    def relu(v):
        pres.append(v)
        a = F.relu(v) if masks is None else _MaskRelu.apply(v, masks[len(acts)].to(dt))
        acts.append(a)
        return a

    h = relu(_gn(F.conv2d(x, sd["0.weight"], None, 2, 3), sd, "1"))
    if pool_idx is None:
        pooled = F.max_pool2d(h, 3, 2, 1)
    else:
        pooled = h.flatten(2).gather(2, pool_idx.flatten(2)).view(pool_idx.shape)
    h = pooled
    for stage in (4, 5, 6, 7):
        for j in (0, 1):
            p = f"{stage}.{j}."
            stride = 2 if (stage > 4 and j == 0) else 1
            idn = h
            if p + "downsample.0.weight" in sd:
                idn = _gn(F.conv2d(h, sd[p + "downsample.0.weight"], None, stride, 0), sd, p + "downsample.1")
            o = relu(_gn(F.conv2d(h, sd[p + "conv1.weight"], None, stride, 1), sd, p + "bn1"))
            h = relu(_gn(F.conv2d(o, sd[p + "conv2.weight"], None, 1, 1), sd, p + "bn2") + idn)
    acts.append(pooled)
    return h.mean(dim=(2, 3)), acts, pres


def heads_ref(sd, feat, finding):
    """{variable: [B, nout]} raw head outputs from the pooled features."""
    out = {}
    for var in VARS:
        w, b = (sd[f"{ENC[var]}.fc.{k}"].detach().to(dtype=feat.dtype, device=feat.device) for k in ("weight", "bias"))
        f = torch.cat([feat, finding.reshape(feat.shape[0], 1).to(feat.dtype)], dim=-1) if var == "age" else feat
        out[var] = F.linear(f, w, b)
    return out


def nll_terms_ref(outs, obs, std_fixed=0.0):
    """{variable: [B]} -log q per sample (flow_pgm.py:659-689)."""
    t = {}
    for var in ("sex", "finding"):
        pc = torch.sigmoid(outs[var]).clamp(EPS32, 1 - EPS32)
        logits = torch.log(pc) - torch.log1p(-pc)
        v = obs[var].reshape(logits.shape).to(logits.dtype)
        t[var] = F.binary_cross_entropy_with_logits(logits, v, reduction="none").sum(-1)
    probs = F.softmax(outs["race"], dim=-1)
    k = obs["race"].max(-1)[1]
    t["race"] = -torch.log(probs.gather(-1, k[:, None]).clamp(EPS32, 1 - EPS32)).sum(-1)
    loc, ls = outs["age"].chunk(2, dim=-1)
    scale = std_fixed * torch.ones_like(ls) if std_fixed > 0 else F.softplus(ls)
    t["age"] = -torch.distributions.Normal(loc, scale).log_prob(obs["age"].reshape(loc.shape).to(loc.dtype)).sum(-1)
    return t


def predict_ref(outs):
    return {"sex": torch.sigmoid(outs["sex"]), "race": F.softmax(outs["race"], dim=-1), "finding": torch.sigmoid(outs["finding"]),
            "age": outs["age"][:, :1]}


def chest_ref(sd, obs, std_fixed=0.0, masks=None, pool_idx=None, dtype=torch.float64):
    """Everything at once in ``dtype`` on the CPU: dict(loss, terms, outs, acts, pres).  obs["x"] may require grad."""
    x = obs["x"].to(dtype)
    o = {k: v.to(dtype) for k, v in obs.items() if k != "x"}
    feat, acts, pres = trunk_ref(sd, x, masks, pool_idx)
    outs = heads_ref(sd, feat, o["finding"])
    terms = nll_terms_ref(outs, o, std_fixed)
    return {"loss": sum(v.sum() for v in terms.values()), "terms": terms, "outs": outs, "acts": acts, "pres": pres}


def randomise(pred, seed):
    """Kaiming-scale conv weights, GroupNorm weight 1 + 0.3 n and bias 0.3 n, head weights at 1 / sqrt(512)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in pred.named_parameters():
            n = torch.randn(p.shape, generator=g)
            if p.dim() == 4:
                p.copy_(n * (2.0 / (p.shape[1] * p.shape[2] * p.shape[3])) ** 0.5)
            elif ".fc." in name:
                p.copy_(n / 512 ** 0.5)
            elif name.endswith("weight"):
                p.copy_(1.0 + 0.3 * n)
            else:
                p.copy_(0.3 * n)
    return pred


def make_obs(B, R, seed):
    """Images uniform in [-1, 1], random observations (CPU, f32)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 1, R, R, generator=g) * 2 - 1
    race = F.one_hot(torch.randint(0, 3, (B,), generator=g), 3).float()
    return {"x": x, "sex": torch.randint(0, 2, (B, 1), generator=g).float(), "race": race,
            "finding": torch.randint(0, 2, (B, 1), generator=g).float(), "age": torch.rand(B, 1, generator=g) * 2 - 1}
