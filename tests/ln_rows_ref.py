"""Plain fp64 restatements of the (dropout ->) residual -> LayerNorm (-> dropout) row kernels of csrc/norm.hip and of their backward.

No GPU, no project import: torch on whatever device the inputs live on.  Everything is widened to fp64 first, so a caller hands in the
(already rounded) fp32 / bf16 values the kernel was given and gets the exact result for those values.
"""
import torch


def _d(t):
    return None if t is None else torch.as_tensor(t).double()


def ln_fwd_ref(x, res, gamma, beta, eps, keep_pre=None, keep_post=None, p_pre=0.0, p_post=0.0):
    """-> (s, mean, rstd, y), fp64.  s = x * keep_pre / (1 - p_pre) + res;  biased variance, eps inside the square root;
    y = (gamma * xhat + beta) * keep_post / (1 - p_post).  keep_* are 0/1 (or bool) masks of x's shape, None = keep everything."""
    s = _d(x)
    if keep_pre is not None:
        s = s * _d(keep_pre) / (1.0 - p_pre)
    if res is not None:
        s = s + _d(res)
    mean = s.mean(-1)
    var = (s - mean.unsqueeze(-1)).pow(2).mean(-1)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = _d(gamma) * ((s - mean.unsqueeze(-1)) * rstd.unsqueeze(-1)) + _d(beta)
    if keep_post is not None:
        y = y * _d(keep_post) / (1.0 - p_post)
    return s, mean, rstd, y


def ln_bwd_ref(dy, s, mean, rstd, gamma, keep_pre=None, keep_post=None, p_pre=0.0, p_post=0.0):
    """-> (ds, dx, dgamma, dbeta), fp64, by the kernel's own contract: xhat is formed from the s, mean and rstd HANDED IN (on the bf16 path s is
    the rounded row while mean / rstd come from the unrounded sum; nothing is recomputed here).
        d = dy * keep_post / (1 - p_post);  g = d * gamma
        ds = rstd * (g - mean_H(g) - xhat * mean_H(g * xhat));  dx = ds * keep_pre / (1 - p_pre)
        dgamma = sum_rows d * xhat;  dbeta = sum_rows d"""
    s, mean, rstd, gamma = _d(s), _d(mean), _d(rstd), _d(gamma)
    H = s.shape[-1]
    xh = (s - mean.unsqueeze(-1)) * rstd.unsqueeze(-1)
    d = _d(dy)
    if keep_post is not None:
        d = d * _d(keep_post) / (1.0 - p_post)
    g = d * gamma
    ds = rstd.unsqueeze(-1) * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    dx = ds if keep_pre is None else ds * _d(keep_pre) / (1.0 - p_pre)
    return ds, dx, (d * xh).reshape(-1, H).sum(0), d.reshape(-1, H).sum(0)


def ln_bwd_col_scales(dy, s, mean, rstd, keep_post=None, p_post=0.0):
    """-> (sum_rows |d * xhat|, sum_rows |d|): the per-column magnitudes the dgamma / dbeta bounds are stated against."""
    s, mean, rstd = _d(s), _d(mean), _d(rstd)
    H = s.shape[-1]
    xh = (s - mean.unsqueeze(-1)) * rstd.unsqueeze(-1)
    d = _d(dy)
    if keep_post is not None:
        d = d * _d(keep_post) / (1.0 - p_post)
    return (d * xh).abs().reshape(-1, H).sum(0), d.abs().reshape(-1, H).sum(0)
