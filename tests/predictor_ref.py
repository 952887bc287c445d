"""f64 torch restatement of the anticausal predictors for the predictor tests: the reference CNN with its BatchNorm unfolded
(layers.py:62-104, eval mode) and the likelihoods of flow_pgm.py's model_anticausal through torch.distributions, with torch's
f32 clamp_probs constant (the reference runs in f32)."""
import copy

import torch
import torch.nn.functional as F

EPS32 = float(torch.finfo(torch.float32).eps)


def cnn_ref(cnn, x, y=None):
    """cnn: a causal_gen_amd.predictor.CNN (or the reference CNN); x, y: f64 tensors on any device."""
    def p(t):
        return t.detach().double().to(x.device)

    h = x
    for i in (0, 4, 7, 10, 13, 16):
        conv, bn = cnn.cnn[i], cnn.cnn[i + 1]
        h = F.conv2d(h, p(conv.weight), None, conv.stride, conv.padding)
        h = F.batch_norm(h, p(bn.running_mean), p(bn.running_var), p(bn.weight), p(bn.bias), False, 0.0, bn.eps)
        h = F.leaky_relu(h, 0.01)
        if i == 0 and isinstance(cnn.cnn[3], torch.nn.MaxPool2d):
            h = F.max_pool2d(h, 2, 2)
    h = h.mean(dim=(-2, -1))
    if y is not None:
        h = torch.cat([h, y], dim=-1)
    fc0, bn, fc3 = cnn.fc[0], cnn.fc[1], cnn.fc[3]
    h = F.leaky_relu(F.batch_norm(F.linear(h, p(fc0.weight)), p(bn.running_mean), p(bn.running_var), p(bn.weight), p(bn.bias), False,
                                  0.0, bn.eps), 0.01)
    return F.linear(h, p(fc3.weight), p(fc3.bias))


def f_scale(ls, std_fixed):
    return std_fixed * torch.ones_like(ls) if std_fixed > 0 else F.softplus(ls)


def normal_nll(out, v, tanh_loc, std_fixed):
    loc, ls = out.chunk(2, dim=-1)
    if tanh_loc:
        loc = torch.tanh(loc)
    return -torch.distributions.Normal(loc, f_scale(ls, std_fixed)).log_prob(v.reshape(loc.shape)).sum()


def categorical_nll(out, onehot):
    probs = F.softmax(out, dim=-1)
    k = onehot.max(-1)[1]
    return -torch.log(probs.gather(-1, k[:, None]).clamp(EPS32, 1 - EPS32)).sum()


def bernoulli_nll(out, v):
    pc = torch.sigmoid(out).clamp(EPS32, 1 - EPS32)
    logits = torch.log(pc) - torch.log1p(-pc)
    return F.binary_cross_entropy_with_logits(logits, v.reshape(logits.shape), reduction="sum")


def predictor_nll(pred, obs, std_fixed=0.0):
    """-sum log q over samples and variables, f64, for a MorphoMNIST / ColourMNIST / Flow predictor; obs["x"] may require grad."""
    x = obs["x"]
    dev = x.device
    o = {k: v.double().to(dev) for k, v in obs.items() if k != "x"}
    B = x.shape[0]
    name = type(pred).__name__
    if name == "MorphoMNISTPredictor":
        return (normal_nll(cnn_ref(pred.encoder_t, x, o["intensity"].reshape(B, 1)), o["thickness"], True, std_fixed)
                + normal_nll(cnn_ref(pred.encoder_i, x), o["intensity"], True, std_fixed)
                + categorical_nll(cnn_ref(pred.encoder_y, x), o["digit"]))
    if name == "ColourMNISTPredictor":
        return categorical_nll(cnn_ref(pred.encoder_y, x), o["digit"]) + categorical_nll(cnn_ref(pred.encoder_c, x), o["colour"])
    val = (normal_nll(cnn_ref(pred.encoder_v, x), o["ventricle_volume"], False, std_fixed)
           + normal_nll(cnn_ref(pred.encoder_b, x, o["ventricle_volume"].reshape(B, 1)), o["brain_volume"], False, std_fixed)
           + bernoulli_nll(cnn_ref(pred.encoder_s, x, o["brain_volume"].reshape(B, 1)), o["sex"])
           + bernoulli_nll(cnn_ref(pred.encoder_m, x), o["mri_seq"]))
    with torch.no_grad():
        ctx = torch.cat([o["brain_volume"].reshape(B, 1), o["ventricle_volume"].reshape(B, 1)], -1)
        a_out = copy.deepcopy(pred.encoder_a).double().to(dev)(ctx)  # (a copy: the module under test keeps its storage)
    return val + normal_nll(a_out, o["age"], False, std_fixed)


def randomise(module, g, scale=1.6):
    """Random weights and non-trivial BatchNorm statistics for a predictor (eval mode)."""
    with torch.no_grad():
        for name, p in module.named_parameters():
            if p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=g) * (scale / p[0].numel() ** 0.5))
            elif name.endswith("weight"):
                p.copy_(0.7 + 0.6 * torch.rand(p.shape, generator=g))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
        for name, b in module.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(0.2 * torch.randn(b.shape, generator=g))
            elif name.endswith("running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=g))
