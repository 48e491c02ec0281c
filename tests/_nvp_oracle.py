"""torch fp64 autograd oracle of ExclusiveKL for an NVPFlow, written literally: sample with g, evaluate log q with the
inverse f, differentiate.  Path form: theta detached inside log q (objectives.py:156-159); plain form: the total
derivative of -mean[log p(g(z0)) - log q(g(z0))], the estimator objectives.py:163 means."""
import math

import numpy as np
import torch

LOG_2PI = math.log(2.0 * math.pi)


def _fold(flow, theta):
    out = {}
    for key, name, off, shape in flow._layout:
        n = int(np.prod(shape))
        out.setdefault(key, {})[name] = theta[off:off + n].reshape(shape)
    return out


def _net(p, n_layers, x, last_tanh):
    for l in range(n_layers):
        x = x @ p[str(l)] + p[str(l) + '_b']
        if l + 1 < n_layers or last_tanh:
            x = torch.tanh(x)
    return x


def g(flow, theta, z):
    p = _fold(flow, theta)
    mask = torch.from_numpy(flow.mask)
    x = z
    for i in range(flow.mask.shape[0]):
        m = mask[i]
        y = x * m
        s = _net(p[str(i) + 's'], len(flow._shapes_s), y, True) * (1 - m)
        t = _net(p[str(i) + 't'], len(flow._shapes_t), y, False) * (1 - m)
        x = y + (1 - m) * (x * torch.exp(s) + t)
    return x


def f(flow, theta, x):
    p = _fold(flow, theta)
    mask = torch.from_numpy(flow.mask)
    z = x
    log_det = torch.zeros(x.shape[0], dtype=torch.float64)
    for i in reversed(range(flow.mask.shape[0])):
        m = mask[i]
        y = m * z
        s = _net(p[str(i) + 's'], len(flow._shapes_s), y, True) * (1 - m)
        t = _net(p[str(i) + 't'], len(flow._shapes_t), y, False) * (1 - m)
        z = (1 - m) * (z - t) * torch.exp(-s) + y
        log_det = log_det - s.sum(dim=1)
    return z, log_det


def prior_log_density(prior, prior_param, z):
    d = prior.dim
    mu = torch.from_numpy(np.asarray(prior_param[:d], dtype=np.float64))
    ls = torch.from_numpy(np.asarray(prior_param[d:], dtype=np.float64))
    r = (z - mu) * torch.exp(-ls)
    if hasattr(prior, 'df'):
        df = float(prior.df)
        const = math.lgamma(0.5 * (df + 1)) - math.lgamma(0.5 * df) - 0.5 * math.log(df * math.pi)
        return torch.sum(const - 0.5 * (df + 1) * torch.log1p(r * r / df) - ls, dim=-1)
    return torch.sum(-0.5 * r * r - ls - 0.5 * LOG_2PI, dim=-1)


def log_density(flow, theta, x):
    z, log_det = f(flow, theta, x)
    return prior_log_density(flow.prior, flow.prior_param, z) + log_det


def model_logp(model, x):
    """torch restatement of the built-in targets used by the tests."""
    import viabel_amd as vb
    if isinstance(model, vb.GaussianModel):
        mean, sd = torch.from_numpy(model.mean), torch.from_numpy(model.stdev)
        r = (x - mean) / sd
        return torch.sum(-0.5 * r * r - torch.log(sd) - 0.5 * LOG_2PI, dim=-1)
    if isinstance(model, vb.FunnelModel):
        k, tau = model.scale_index, model.log_sigma_stdev
        v = x[:, k]
        lp_v = -0.5 * (v / tau) ** 2 - math.log(tau) - 0.5 * LOG_2PI
        keep = [j for j in range(x.shape[1]) if j != k]
        o = x[:, keep]
        lp_o = torch.sum(-0.5 * o ** 2 * torch.exp(-2.0 * v)[:, None] - v[:, None] - 0.5 * LOG_2PI, dim=1)
        return lp_v + lp_o
    if isinstance(model, vb.CorrelatedGaussianModel):
        mean, P = torch.from_numpy(model.mean), torch.from_numpy(model.precision)
        c = x - mean
        return -0.5 * torch.sum((c @ P) * c, dim=1) + 0.5 * model.logdet_precision - 0.5 * x.shape[1] * LOG_2PI
    logp = getattr(model, '_torch_logp', None)
    if logp is None:
        raise TypeError('no torch restatement of %r' % type(model).__name__)
    return logp(x)


def objective(flow, model, theta, z0, path):
    """(value, grad) of ExclusiveKL on the prior draws z0 (N x D)."""
    th = torch.tensor(np.asarray(theta, dtype=np.float64), requires_grad=True)
    z = torch.from_numpy(np.asarray(z0, dtype=np.float64))
    x = g(flow, th, z)
    logq = log_density(flow, th.detach() if path else th, x)
    value = -torch.mean(model_logp(model, x) - logq)
    value.backward()
    return float(value.detach()), th.grad.numpy().copy()
