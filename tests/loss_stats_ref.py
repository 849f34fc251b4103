"""fp64 numpy restatement of the two stats losses (ops.cross_entropy_stats, ops.kl_masked_stats): loss, gradient, row arg-max, hits, counts.

Written from the definitions, not from the kernels:
  CE row loss  = (1 - eps) (lse - x[t]) + eps (lse - mean of the row's logits that are not -inf)          -- the FINITE-CLASS smoothing rule:
                 with no -inf in the row this is F.cross_entropy(label_smoothing=eps); a -inf logit takes no share of the smoothing mass
  d / d x[c]   = (p_c - (1 - eps) [c == t] - (eps / nv) [x_c != -inf]) / count
  arg-max      = np.argmax: the lowest index among equal maxima, and a NaN counts as the maximum (the first NaN wins) -- torch.argmax's rule
  KL row loss  = mask * sum_c t_c (log t_c - log_softmax(x)_c) over t_c > 0, divided by max(1, sum(mask))
"""
import numpy as np


def _lse(x):
    """log-sum-exp of the rows of x; -inf for a row of -inf, NaN for a row holding a NaN"""
    with np.errstate(all="ignore"):
        m = np.max(x, axis=-1, keepdims=True)
        safe = np.where(np.isneginf(m), 0.0, m)
        return (safe + np.log(np.sum(np.exp(x - safe), axis=-1, keepdims=True)))[..., 0]


def ce_stats(x, target, ignore_index=-100, eps=0.0, gout=1.0):
    """x [M, V], target [M] -> dict(loss, grad [M, V], row_loss [M], row_top [M] int64, hits, count)."""
    x = np.asarray(x, dtype=np.float64)
    target = np.asarray(target, dtype=np.int64)
    M, V = x.shape
    live = target != ignore_index
    count = int(live.sum())
    row_loss, row_top, grad = np.zeros(M), np.full(M, -1, dtype=np.int64), np.zeros((M, V))
    with np.errstate(all="ignore"):
        for r in np.nonzero(live)[0]:
            t, xr = int(target[r]), x[r]
            row_top[r] = int(np.argmax(xr))
            if not 0 <= t < V:
                row_loss[r], grad[r] = np.nan, np.nan
                continue
            finite = ~np.isneginf(xr)                      # "finite" = not -inf (a NaN or +inf stays in, and poisons)
            nv = int(finite.sum())
            lse = float(_lse(xr[None])[0])
            nll = lse - xr[t]
            row_loss[r] = nll if eps == 0.0 else (1.0 - eps) * nll + eps * (lse - xr[finite].sum() / nv)
            g = np.exp(xr - lse)
            g[t] -= 1.0 - eps
            if eps != 0.0:
                g[finite] -= eps / nv
            grad[r] = g * (gout / count)
        loss = row_loss.sum() / count if count else np.nan
    hits = int((live & (row_top == target)).sum())
    return dict(loss=loss, grad=grad, row_loss=row_loss, row_top=row_top, hits=hits, count=count)


def kl_stats(x, target, mask, gout=1.0):
    """x, target [M, C], mask [M] int -> dict(loss, grad [M, C], row_top [M] int64, hits, count)."""
    x = np.asarray(x, dtype=np.float64)
    tg = np.asarray(target, dtype=np.float64)
    mask = np.asarray(mask, dtype=np.int64)
    M, C = x.shape
    on = mask != 0
    denom = max(1.0, float(mask.sum()))
    with np.errstate(all="ignore"):
        logp = x - _lse(x)[:, None]
        terms = np.where(tg > 0, tg * (np.log(np.where(tg > 0, tg, 1.0)) - logp), 0.0)
        loss = float(np.where(on, terms.sum(-1) * mask, 0.0).sum() / denom)          # an unmasked row is never read
        grad = (np.exp(logp) * tg.sum(-1, keepdims=True) - tg) * (mask[:, None] * (gout / denom))
    grad[~on] = 0.0
    top = np.argmax(x, axis=-1).astype(np.int64)
    hits = int((on & (top == np.argmax(tg, axis=-1))).sum())
    return dict(loss=loss, grad=grad, row_top=np.where(on, top, -1), hits=hits, count=int(on.sum()))
