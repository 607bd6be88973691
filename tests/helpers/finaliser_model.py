"""float64 models, in plain torch on the CPU, of what the end-of-pass finalisers and their neighbours compute (csrc/finalise.hip,
norm.hip's two-launch backward, spectral.hip's power iteration and dv).  Every function takes the kernels' fp32 inputs widened to
double and calls nothing but torch: tests/test_finaliser_model.py holds them to float64 autograd, tests/test_gpu_finalisers.py
and tests/test_gpu_deferred_layers.py hold the kernels to them."""
import torch


def _d(t):
    return torch.as_tensor(t).detach().double().cpu()


def root_tanh(o):
    return (o * o + 1).pow(0.25) * torch.tanh(o)


def root_tanh_grad(o):
    """d/do of (o^2 + 1)^(1/4) tanh o (libs/activation.py:22-36)."""
    q = o * o + 1
    sech2 = torch.cosh(o).pow(-2)
    return (2 * q * sech2 + o * torch.tanh(o)) / (2 * q.pow(0.75))


def _norm_operands(x, scale, bias, per_sample):
    x = _d(x)
    B, C = x.shape[0], x.shape[1]
    scale = _d(scale).reshape(B if per_sample else 1, C, 1)
    bias = _d(bias).reshape(1, C, 1)
    return x.reshape(B, C, -1), scale, bias


def norm_fwd(x, scale, bias, per_sample, groups, with_act):
    """InPlaceNorm forward (libs/inplace_norm.py:4-45): each of the `groups` equal batch slices has its own scalar mean and
    unbiased std.  Returns (out, stats [groups, 2] = {mean, std})."""
    shape = torch.as_tensor(x).shape
    x, scale, bias = _norm_operands(x, scale, bias, per_sample)
    Bg = x.shape[0] // groups
    out = torch.empty_like(x)
    stats = torch.empty(groups, 2, dtype=torch.float64)
    for k in range(groups):
        sl = slice(k * Bg, (k + 1) * Bg)
        xs = x[sl]
        mu = xs.mean()
        sd = ((xs - mu).pow(2).sum() / (xs.numel() - 1)).sqrt()
        o = (xs - mu) * (scale[sl] if per_sample else scale) / sd + bias
        out[sl] = root_tanh(o) if with_act else o
        stats[k, 0], stats[k, 1] = mu, sd
    return out.reshape(shape), stats


def norm_bwd(x, g, scale, bias, per_sample, groups, with_act):
    """Backward of norm_fwd incl. the path through std.  Returns (dx, dscale, dbias, stats); dscale [B, C, 1, 1] (per sample) or
    [1, C, 1, 1] and dbias [1, C, 1, 1] are summed over all slices (include/locate_hip.h: "dscale / dbias sum over all groups")."""
    shape = torch.as_tensor(x).shape
    x, scale, bias = _norm_operands(x, scale, bias, per_sample)
    g = _d(g).reshape(x.shape)
    B, C = x.shape[0], x.shape[1]
    Bg = B // groups
    dx = torch.empty_like(x)
    dscale = torch.zeros_like(scale)
    dbias = torch.zeros_like(bias)
    stats = torch.empty(groups, 2, dtype=torch.float64)
    for k in range(groups):
        sl = slice(k * Bg, (k + 1) * Bg)
        xs, go = x[sl], g[sl]
        ys = scale[sl] if per_sample else scale
        n = xs.numel()
        mu = xs.mean()
        xc = xs - mu
        sd = (xc.pow(2).sum() / (n - 1)).sqrt()
        if with_act:
            go = go * root_tanh_grad(xc * ys / sd + bias)
        yg = ys * go / sd
        dz = -(xc * go * ys).sum() / (sd * sd)
        dx[sl] = yg - yg.mean() + dz * xc / ((n - 1) * sd)
        ds = (xc * go / sd).sum(2, keepdim=True)
        if per_sample:
            dscale[sl] = ds
        else:
            dscale += ds.sum(0, keepdim=True)
        dbias += go.sum((0, 2), keepdim=True)
        stats[k, 0], stats[k, 1] = mu, sd
    return dx.reshape(shape), dscale.unsqueeze(-1), dbias.unsqueeze(-1), stats


def sn_rank1(gw_in, partial, u, v, sigma_tab, wv, groups):
    """The rank-1 term of d(W_bar / sigma), du and dsigma, for both meanings of a rank-1 record.
    groups = 0 (one call): partial [np] sums to <G, W_bar> of the UNSCALED weight gradient, sigma_tab = {sigma, 1/sigma}, wv [h]:
        dsigma = -sum(partial) / sigma^2,  du = dsigma wv.
    groups = k >= 1 (stacked calls): partial [k, np], row j sums to <gy_j, y_j - bias>, sigma_tab [k, >= 2] = {sigma_j, ...}, wv [k, h]:
        dsigma_j = -sum_j / sigma_j,  du = sum_j dsigma_j wv_j.
    Either way gw = gw_in + (sum_j dsigma_j) u v^T with the CURRENT u, v.  Returns (gw, du, dsigma_total)."""
    gw_in, partial, u, v, sigma_tab, wv = (_d(t) for t in (gw_in, partial, u, v, sigma_tab, wv))
    h, wd = u.numel(), v.numel()
    if groups == 0:
        sigma = sigma_tab.reshape(-1)[0]
        total = -partial.sum() / (sigma * sigma)
        du = total * wv.reshape(-1)[:h]
    else:
        sums = partial.reshape(groups, -1).sum(1)
        dsig = -sums / sigma_tab.reshape(groups, -1)[:, 0]
        total = dsig.sum()
        du = (dsig[:, None] * wv.reshape(groups, -1)[:, :h]).sum(0)
    gw = gw_in.reshape(h, wd) + total * torch.outer(u, v)
    return gw.reshape(gw_in.shape), du, total


def sn_dots(gy, y, bias, groups):
    """Per stacked call j: <gy_j, y_j - bias> and, beside it, the sum of magnitudes sum |gy (y - bias)| (what a tolerance on the
    dot is a fraction of).  gy, y [groups * Bg, M, ...]; bias [M] or None."""
    gy, y = _d(gy), _d(y)
    B, M = gy.shape[0], gy.shape[1]
    gy, y = gy.reshape(B, M, -1), y.reshape(B, M, -1)
    if bias is not None:
        y = y - _d(bias).reshape(1, M, 1)
    prod = (gy * y).reshape(groups, -1)
    return prod.sum(1), prod.abs().sum(1)


def channel_sums(g):
    """out[c] = sum over batch and space of g[:, c] (a bias gradient), and the sum of magnitudes beside it."""
    g = _d(g)
    g = g.reshape(g.shape[0], g.shape[1], -1)
    return g.sum((0, 2)), g.abs().sum((0, 2))


def power_iteration(W, u, eps=1e-12):
    """One power iteration (libs/spectral_norm.py:21-32; csrc/spectral.hip:3): returns (u', v', sigma, wv = W v')."""
    W, u = _d(W), _d(u)
    W = W.reshape(u.numel(), -1)
    t = W.t().mv(u)
    v = t / (t.norm() + eps)
    wv = W.mv(v)
    u2 = wv / (wv.norm() + eps)
    return u2, v, u2.dot(wv), wv


def dv(W, u, slots):
    """dv = (sum of the layer's dsigma slots) * W^T u."""
    W, u = _d(W), _d(u)
    return _d(slots).sum() * W.reshape(u.numel(), -1).t().mv(u)
