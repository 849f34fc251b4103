"""tests/ln_rows_ref.py (the fp64 reference the LayerNorm row-kernel tests judge against) is itself checked against fp64 autograd of
torch.nn.functional.layer_norm, with and without fixed dropout masks, and for the one point where it deliberately differs from autograd: the
backward uses the statistics it is handed."""
import pytest
import torch
import torch.nn.functional as F

from ln_rows_ref import ln_bwd_col_scales, ln_bwd_ref, ln_fwd_ref

EPS = 1e-12


def _inputs(H, rows=5, seed=0):
    g = torch.Generator().manual_seed(1000 * H + seed)
    x, res, dy = (torch.randn(rows, H, generator=g, dtype=torch.float64) for _ in range(3))
    gamma = 1 + 0.1 * torch.randn(H, generator=g, dtype=torch.float64)
    beta = 0.1 * torch.randn(H, generator=g, dtype=torch.float64)
    kp = (torch.rand(rows, H, generator=g) >= 0.25).double()
    kq = (torch.rand(rows, H, generator=g) >= 0.1).double()
    return x, res, dy, gamma, beta, kp, kq


def _close(a, b, what):
    err = float((a - b).abs().max())
    assert err <= 1e-12 * max(1.0, float(b.abs().max())), (what, err)


@pytest.mark.parametrize("H", [4, 36, 260])
@pytest.mark.parametrize("masks", ["none", "pre", "post", "both"])
def test_reference_equals_fp64_autograd(H, masks):
    x, res, dy, gamma, beta, kp, kq = _inputs(H)
    keep_pre = kp if masks in ("pre", "both") else None
    keep_post = kq if masks in ("post", "both") else None
    p_pre, p_post = (0.25 if keep_pre is not None else 0.0), (0.1 if keep_post is not None else 0.0)
    xa, ra, ga, ba = (t.clone().requires_grad_(True) for t in (x, res, gamma, beta))
    sa = (xa * keep_pre / (1 - p_pre) if keep_pre is not None else xa) + ra          # dropout_mask . x + res
    ya = F.layer_norm(sa, (H,), ga, ba, EPS)                                          # -> layer_norm
    if keep_post is not None:
        ya = ya * keep_post / (1 - p_post)                                            # -> . mask
    ya.backward(dy)
    s, mean, rstd, y = ln_fwd_ref(x, res, gamma, beta, EPS, keep_pre, keep_post, p_pre, p_post)
    _close(s, sa.detach(), "s")
    _close(y, ya.detach(), "y")
    _close(mean, sa.detach().mean(-1), "mean")
    _close(rstd, 1 / torch.sqrt(sa.detach().var(-1, unbiased=False) + EPS), "rstd")
    ds, dx, dg, db = ln_bwd_ref(dy, s, mean, rstd, gamma, keep_pre, keep_post, p_pre, p_post)
    _close(ds, ra.grad, "ds")
    _close(dx, xa.grad, "dx")
    _close(dg, ga.grad, "dgamma")
    _close(db, ba.grad, "dbeta")
    if keep_pre is not None:
        assert bool((dx[keep_pre == 0] == 0).all())
    sg, sb = ln_bwd_col_scales(dy, s, mean, rstd, keep_post, p_post)
    assert bool((sg >= dg.abs() - 1e-12).all()) and bool((sb >= db.abs() - 1e-12).all())


def test_reference_without_residual_and_constant_row():
    H = 36
    x, _, dy, gamma, beta, _, _ = _inputs(H)
    x[2] = 2.5
    s, mean, rstd, y = ln_fwd_ref(x, None, gamma, beta, EPS)
    assert torch.equal(s, x)
    _close(y, F.layer_norm(x, (H,), gamma, beta, EPS), "y")
    _close(y[2], beta, "a constant row gives beta")
    assert float(rstd[2]) == pytest.approx(1e6, rel=1e-9)


def test_both_dropouts_in_one_call_are_refused_before_anything_is_launched():
    """One call draws one mask (tests/test_ln_rows_dispatch_gpu.py has the kernel side): the combination raises before any tensor is looked at."""
    from ytvln import ops
    x = torch.zeros(2, 8)
    with pytest.raises(RuntimeError, match="both > 0"):
        ops.add_layer_norm(x, None, torch.ones(8), torch.zeros(8), 1e-12, 0.25, 0.25, object())
    with pytest.raises(RuntimeError, match="both > 0"):
        ops.AddLayerNormFn.apply(x, None, torch.ones(8), torch.zeros(8), 1e-12, 0.25, 0.1, None, 0)


@pytest.mark.parametrize("H", [4, 36, 260])
def test_backward_uses_the_statistics_it_is_handed(H):
    x, res, dy, gamma, beta, _, _ = _inputs(H, seed=1)
    s, mean, rstd, _ = ln_fwd_ref(x, res, gamma, beta, EPS)
    ds0, _, dg0, db0 = ln_bwd_ref(dy, s, mean, rstd, gamma)
    ds1, _, dg1, db1 = ln_bwd_ref(dy, s, mean + 0.1, rstd, gamma)
    ds2, _, dg2, _ = ln_bwd_ref(dy, s, mean, rstd * 1.5, gamma)
    assert float((ds1 - ds0).abs().max()) > 1e-3 and float((dg1 - dg0).abs().max()) > 1e-3
    assert float((ds2 - ds0).abs().max()) > 1e-3 and float((dg2 - dg0).abs().max()) > 1e-3
    assert torch.equal(db1, db0)                      # dbeta does not involve the statistics
    # ... and follows its formula for arbitrary statistics: restated element by element for one row
    g = torch.Generator().manual_seed(H)
    m, r = torch.randn(s.shape[0], generator=g, dtype=torch.float64), 0.5 + torch.rand(s.shape[0], generator=g, dtype=torch.float64)
    ds, _, _, _ = ln_bwd_ref(dy, s, m, r, gamma)
    xh = (s[1] - m[1]) * r[1]
    gg = dy[1] * gamma
    want = r[1] * (gg - gg.sum() / H - xh * (gg * xh).sum() / H)
    _close(ds[1], want, "ds with arbitrary statistics")
