"""Every instantiation of the LayerNorm row kernels (csrc/norm.hip), judged PER ROW against fp64 (tests/ln_rows_ref.py) through the C ABI.

A launch of the (dropout ->) residual -> LayerNorm (-> dropout) forward or of its backward picks one of 22 kernel instantiations from H, the row
type and, for bf16 rows, the alignment of the row pointers.  The table, as read from csrc/norm.hip:

  path                                         selector (norm.hip lines)                                          instantiations
  ln_fwd_kernel<NV, MODE, XT, YT>   (61-163)   launch_ln, 786-795: nv = cdiv(H / 4, 64); grid = min(cdiv(rows, 4),  NV 1 (H <= 256), 2 (<= 512),
    4 elements per lane and vector              4096) workgroups of 4 rows, so the row loop takes a second trip      4 (<= 1024), 8 (<= 2048)
                                                above 16384 rows
  ln_bwd_kernel<NV, XT>             (171-265)   ytvln_ln_bwd_f32, 867-891: the same nv; nb = ytvln_ln_bwd_blocks      NV 1, 2, 4, 8
                                                (865) = min(768, cdiv(rows, 4)), rows_per_block = cdiv(rows, nb);
                                                a block with r0 >= rows still writes a zero partial record
  ln_fwd_bf16x8_kernel<NV>          (302-387)   ytvln_ln_fwd_bf16, 1021-1027: bf16 rows, H % 8 == 0 and x / res /    NV 1 (H <= 512), 2 (<= 1024),
    8 elements per lane and vector              y / s_out 16-byte aligned; nv = cdiv(H / 8, 64); grid = min(cdiv     4 (<= 2048)
                                                (rows, 4), nv <= 2 ? 1024 : 512): second trip above 4096 / 2048 rows
  ln_bwd_bf16x8_kernel<NV>          (389-489)   ytvln_ln_bwd_bf16, 1088-1092: H % 8 == 0 and dy / s / ds / dx        NV 1, 2, 4
                                                16-byte aligned; nv8 = cdiv(H / 8, 64)
  bf16 rows on the 4-wide kernels               1028-1029 and 1096-1099: H % 8 == 4 (32-bit dropout draws), or       NV 1, 2, 4, 8 of
    ln_fwd_kernel<NV, LN_PLAIN, bf16_t, bf16_t>  H % 8 == 0 with a row pointer that is only 8-byte aligned (the      each of the two kernels
    ln_bwd_kernel<NV, bf16_t>                    16-bit draws of the 8-wide kernels: drop4 with x8, 47-59)
  embedding forwards                            launch_ln<LN_TEXT / LN_IMAGE> (838, 858, 1047, 1065): the NV table
                                                of ln_fwd_kernel

One parametrised case of test_rows_forward_backward runs the forward AND the backward of its class, so these ids reach the 22 instantiations:

  ln_fwd_kernel / ln_bwd_kernel, fp32 rows      <1> f32-nv1-H252-r7     <2> f32-nv2-H384-r7     <4> f32-nv4-H1020-r7    <8> f32-nv8-H1536-r7
  ln_fwd_bf16x8_kernel / ln_bwd_bf16x8_kernel   <1> bf16x8-nv1-H264-r7  <2> bf16x8-nv2-H1016-r7 <4> bf16x8-nv4-H1544-r7
  ln_fwd_kernel / ln_bwd_kernel, bf16 rows      <1> bf16w4-nv1-H36-r7   <2> bf16w4-nv2-H260-r7  <4> bf16w4-nv4-H516-r7  <8> bf16w4-nv8-H2044-r7
    ... reached through the alignment fallback  <1> bf16off-nv1-H8-r7   <2> bf16off-nv2-H512-r7 <4> bf16off-nv4-H1024-r7 <8> bf16off-nv8-H2048-r7
  (4 + 4) + (3 + 3) + (4 + 4) = 22; the other ids are the two sides of every boundary of the table and the row counts 1 and 7.

Bars.  Inputs are drawn as in test_layernorm_full_grids_every_row_right_and_reproducible (randn rows, gamma = 1 + 0.1 randn, beta = 0.1 randn) and
the fp32 bars are that test's: per row, max |y - ref| <= D_Y = 2e-5 and max |ds - ref| <= D_DS = 1e-4.  bf16 outputs are held element by element
to |out - ref| <= 2^-8 |ref| + 2 delta: half the spacing of a 7-bit mantissa under round-to-nearest-even, plus the fp32 arithmetic in front of
the rounding, which may carry a value across a rounding boundary (delta = D_Y for y, D_DS for ds, dx and s_out).  The reference is always the
fp64 result for the rounded values the kernel was handed.  mean / rstd: 1e-6 relative + 1e-6 absolute.  dgamma / dbeta: the fp32 [nb, 2, H]
partial records summed on the host in fp64, per COLUMN |got - ref| <= 1e-5 sum_rows |d xhat| (resp. sum_rows |d|) + 1e-6.  No case needed a bar
of its own (H = 4, with its four-element variance, included).

The backward is fed ARBITRARY statistics (mean = 0.3 randn, rstd in [0.5, 1.5), not those of s), so the test binds the formula -- xhat from the
s, mean and rstd handed in -- and not a forward / backward pair; the dropout tests run real pairs.

Form pairs.  For bf16 rows with H % 8 == 0 the forward and the backward each exist 8-wide (aligned) and 4-wide (a pointer 8 bytes off), and all
four combinations must regenerate the same masks: asserted exactly, together with bit-identical s_out (no reduction is involved in it).  y, ds
and dx are NOT bit-identical between the forms, and are held to the per-row bars instead: a lane of the 4-wide kernel owns elements
4 (lane + 64 j) .. + 3, a lane of the 8-wide kernel 8 (lane + 64 j) .. + 7, so the two sum a row in different orders (mean, variance and the two
backward row sums differ in the last bits), and the 4-wide forward divides by sqrt(var + eps) where the 8-wide one multiplies by its reciprocal.

What this module found: the forward kernels formed the mean as sum * (1 / H) with the rounded reciprocal.  For a constant row of 2.5 that is
2.5000002 at H = 252 and H = 1020 (exact at every other H below), and with eps = 1e-12 that one ulp is the whole variance: xhat = -0.23 instead
of 0, y = beta - 0.23 gamma (f32-nv1-H252-r7 and f32-nv4-H1020-r7 measured a row error of 0.30 on that build, every other case passed).  The
kernels now divide (sum / H: the row sum of a constant row is exact, so is the correctly rounded quotient, as in the reference's x.mean(-1)).
"""
import math

import pytest
import torch

from helpers import rel_l2
from ln_rows_ref import ln_bwd_col_scales, ln_bwd_ref, ln_fwd_ref

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EPS = 1e-12
D_Y, D_DS = 2e-5, 1e-4
GUARD = 64              # guard elements on either side of every carved buffer (a multiple of 16 bytes in both row types)
SENTINEL = -3.0         # exact in fp32 and bf16
OFF = 4                 # elements: 8 bytes into a bf16 row buffer -- 8-byte but not 16-byte aligned, and H % 8 == 0 keeps every row there
SITE = 5

# kind -> (bf16 rows, element offset of every row pointer)
KINDS = {"f32": (False, 0), "bf16x8": (True, 0), "bf16w4": (True, 0), "bf16off": (True, OFF)}


def _nv(kind, H):
    per = 8 if kind == "bf16x8" else 4
    n = -(-(H // per) // 64)
    return 1 if n <= 1 else 2 if n <= 2 else 4 if (n <= 4 or per == 8) else 8


def _case(kind, H, rows):
    return pytest.param(kind, H, rows, id=f"{kind}-nv{_nv(kind, H)}-H{H}-r{rows}")


WIDTHS = {"f32": (4, 252, 256, 260, 384, 512, 516, 1020, 1028, 1536, 2044, 2048),
          "bf16x8": (8, 264, 512, 520, 1016, 1032, 1544, 2048),
          "bf16w4": (4, 36, 260, 508, 516, 1028, 2044),
          "bf16off": (8, 512, 1024, 2048)}
ROW_CASES = [_case(k, H, r) for k, hs in WIDTHS.items() for H in hs for r in (1, 7)]
# the smallest row counts that reach the second trip of each forward row loop, at one narrow and one wide H of the form
FWD_LOOP_CASES = [_case("f32", 32, 16391), _case("f32", 260, 16391), _case("bf16x8", 8, 4101), _case("bf16x8", 520, 4101),
                  _case("bf16x8", 1032, 2055), _case("bf16x8", 2048, 2055)]
# backward: nb = 768, rows_per_block = 5, blocks 616..767 own no row
BWD_EMPTY_CASES = [_case("f32", 260, 3077), _case("bf16x8", 520, 3077)]
# one H per class for the dropout masks
MASK_WIDTHS = {"f32": (252, 384, 1020, 1536), "bf16x8": (264, 1016, 1544), "bf16w4": (36, 260, 516, 1028), "bf16off": (8, 512, 1024, 2048)}
MASK_CASES = [pytest.param(k, H, p, side, id=f"{k}-nv{_nv(k, H)}-H{H}-p{p}-{side}")
              for k, hs in MASK_WIDTHS.items() for H in hs for p in (0.25, 0.1) for side in ("pre", "post")]


# ------------------------------------------------------------------------------------------------------------------
# plumbing: carved buffers, launches, bars
# ------------------------------------------------------------------------------------------------------------------
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sync():
    torch.cuda.synchronize()


class Slot:
    """`shape` elements of `dtype` carved out of a larger buffer at GUARD + off elements: the test owns the pointer, its alignment and what lies
    on either side of it.  Outputs (src = None) are poisoned with NaN; the guard elements hold SENTINEL."""

    def __init__(self, dev, dtype, shape, off=0, src=None):
        n = math.prod(shape)
        self.buf = torch.full((GUARD + off + n + GUARD,), SENTINEL, dtype=dtype, device=dev)
        self.lo, self.hi = GUARD + off, GUARD + off + n
        self.t = self.buf[self.lo:self.hi].view(shape)
        if src is None:
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(src)
        self.ptr = self.t.data_ptr()
        assert self.buf.data_ptr() % 16 == 0 and self.ptr % 16 == (off * self.buf.element_size()) % 16

    def check(self, what):
        assert bool((self.buf[:self.lo] == SENTINEL).all()) and bool((self.buf[self.hi:] == SENTINEL).all()), f"{what}: guard elements overwritten"
        assert bool(torch.isfinite(self.t).all()), f"{what}: {int((~torch.isfinite(self.t)).sum())} elements not written (or not finite)"
        return self.t


def _ptr(t):
    return None if t is None else (t.ptr if isinstance(t, Slot) else t.data_ptr())


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16 if a.dtype == BF else torch.int32), b.view(torch.int16 if b.dtype == BF else torch.int32))


def launch_fwd(x, res, gamma, beta, off=0, p_pre=0.0, p_post=0.0, rng=None, site=0):
    """Two launches of ytvln_ln_fwd_<row type> into fresh poisoned buffers -> (y, s_out, mean, rstd) of the first, after checking that every
    output element was written, no guard element was, and that the second launch gave the same bits."""
    from ytvln import _lib
    dev, (rows, H), bf = x.device, x.shape, x.dtype == BF
    X = Slot(dev, x.dtype, (rows, H), off, x)
    R = Slot(dev, x.dtype, (rows, H), off, res) if res is not None else None
    runs = []
    for _ in range(2):
        out = [Slot(dev, x.dtype, (rows, H), off), Slot(dev, x.dtype, (rows, H), off), Slot(dev, torch.float32, (rows,)), Slot(dev, torch.float32, (rows,))]
        _lib.call("ytvln_ln_fwd_bf16" if bf else "ytvln_ln_fwd_f32", _ptr(X), _ptr(R), _ptr(gamma), _ptr(beta), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                  _ptr(out[3]), rows, H, EPS, float(p_pre), float(p_post), _ptr(rng), site, _stream())
        runs.append(out)
    _sync()
    got = [[s.check(f"ln_fwd {n}") for s, n in zip(run, ("y", "s_out", "mean", "rstd"))] for run in runs]
    for a, b, n in zip(got[0], got[1], ("y", "s_out", "mean", "rstd")):
        assert _same_bits(a, b), f"ln_fwd {n}: two launches differ"
    assert bool((X.buf[:X.lo] == SENTINEL).all()) and torch.equal(X.t, x), "ln_fwd wrote into its input"
    return got[0]


def launch_bwd(dy, s, mean, rstd, gamma, off=0, p_pre=0.0, p_post=0.0, rng=None, site=0):
    """Two launches of ytvln_ln_bwd_<row type> -> (ds, dx | None, partial [nb, 2, H]); bf16 rows also take the fp32 copy of ds, which must be the
    unrounded ds: it rounds to ds bit for bit."""
    from ytvln import _lib
    dev, (rows, H), bf = dy.device, dy.shape, dy.dtype == BF
    DY, S = Slot(dev, dy.dtype, (rows, H), off, dy), Slot(dev, dy.dtype, (rows, H), off, s)
    nb = _lib.load().ytvln_ln_bwd_blocks(rows)
    assert nb == max(1, min(768, -(-rows // 4)))
    runs = []
    for _ in range(2):
        ds, dx = Slot(dev, dy.dtype, (rows, H), off), (Slot(dev, dy.dtype, (rows, H), off) if p_pre > 0 else None)
        ds32 = Slot(dev, torch.float32, (rows, H)) if bf else None
        part = Slot(dev, torch.float32, (nb, 2, H))
        _lib.call("ytvln_ln_bwd_bf16" if bf else "ytvln_ln_bwd_f32", _ptr(DY), _ptr(S), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(ds), _ptr(dx),
                  *((_ptr(ds32),) if bf else ()), _ptr(part), rows, H, float(p_pre), float(p_post), _ptr(rng), site, _stream())
        runs.append((ds, dx, ds32, part))
    _sync()
    names = ("ds", "dx", "ds_f32", "partial")
    got = [[None if s is None else s.check(f"ln_bwd {n}") for s, n in zip(run, names)] for run in runs]
    for a, b, n in zip(got[0], got[1], names):
        assert a is None or _same_bits(a, b), f"ln_bwd {n}: two launches differ"
    ds, dx, ds32, part = got[0]
    if bf:
        assert _same_bits(ds32.to(BF), ds), "ln_bwd: the fp32 copy of ds does not round to ds"
    return ds, dx, part


def check_rows(got, ref, delta, what):
    """fp32 rows: per row max |got - ref| <= delta.  bf16 rows: every element within 2^-8 |ref| + 2 delta (see the module docstring)."""
    err = (got.double() - ref).abs()
    over = err - (2.0 ** -8 * ref.abs() + 2 * delta) if got.dtype == BF else err - delta
    worst = over.reshape(over.shape[0], -1).amax(-1)          # per row
    print(f"{what}: worst row error {float(err.max()):.3e}, margin {-float(worst.max()):.3e}")
    assert float(worst.max()) <= 0.0, (what, float(err.max()), (worst > 0).nonzero().flatten()[:6].tolist(), int((worst > 0).sum()))


def check_stats(got, ref, what):
    err = (got.double() - ref).abs()
    assert bool((err <= 1e-6 * ref.abs() + 1e-6).all()), (what, float(err.max()), float((err / ref.abs().clamp_min(1e-30)).max()))


def check_gamma_beta(part, dy, s, mean, rstd, gamma, keep_post=None, p_post=0.0):
    _, _, dg, db = ln_bwd_ref(dy, s, mean, rstd, gamma, None, keep_post, 0.0, p_post)
    sg, sb = ln_bwd_col_scales(dy, s, mean, rstd, keep_post, p_post)
    got = part.double().sum(0)          # [2, H]: the fp32 partial records, summed in fp64
    for g, r, sc, n in ((got[0], dg, sg, "dgamma"), (got[1], db, sb, "dbeta")):
        err = (g - r).abs()
        assert bool((err <= 1e-5 * sc + 1e-6).all()), (n, float(err.max()), (err > 1e-5 * sc + 1e-6).nonzero().flatten()[:6].tolist())
    return got


def draw(dev, kind, H, rows, seed=0, beta_mean=0.0):
    """randn rows of the kind's row type (rounded once), fp32 gamma = 1 + 0.1 randn and beta = beta_mean + 0.1 randn, arbitrary backward statistics"""
    g = torch.Generator().manual_seed(1000003 * seed + 4099 * H + rows)
    cast = (lambda t: t.to(BF)) if KINDS[kind][0] else (lambda t: t)
    x, res, dy = (cast(torch.randn(rows, H, generator=g).to(dev)) for _ in range(3))
    gamma = (1 + 0.1 * torch.randn(H, generator=g)).to(dev)
    beta = (beta_mean + 0.1 * torch.randn(H, generator=g)).to(dev)
    mean_a = (0.3 * torch.randn(rows, generator=g)).to(dev)
    rstd_a = (0.5 + torch.rand(rows, generator=g)).to(dev)
    return x, res, dy, gamma, beta, mean_a, rstd_a


def check_forward(kind, x, res, gamma, beta, const_row=None):
    off = KINDS[kind][1]
    y, s, mean, rstd = launch_fwd(x, res, gamma, beta, off)
    sr, mr, rr, yr = ln_fwd_ref(x, res, gamma, beta, EPS)
    check_rows(y, yr, D_Y, "y")
    check_rows(s, sr, D_DS, "s_out")
    check_stats(mean, mr, "mean")
    check_stats(rstd, rr, "rstd")
    if const_row is not None:          # variance 0, eps inside the square root: y = beta
        check_rows(y[const_row:const_row + 1], beta.double().unsqueeze(0), D_Y, "y of the constant row")
    return y, s, mean, rstd


def check_backward(kind, dy, s, mean, rstd, gamma):
    ds, _, part = launch_bwd(dy, s, mean, rstd, gamma, KINDS[kind][1])
    dsr, _, _, _ = ln_bwd_ref(dy, s, mean, rstd, gamma)
    check_rows(ds, dsr, D_DS, "ds")
    check_gamma_beta(part, dy, s, mean, rstd, gamma)
    return part


# ------------------------------------------------------------------------------------------------------------------
# every class, both sides of every boundary
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,H,rows", ROW_CASES)
def test_rows_forward_backward(dev, lib, kind, H, rows):
    x, res, dy, gamma, beta, mean_a, rstd_a = draw(dev, kind, H, rows)
    const_row = None
    if rows == 7:
        const_row = 3
        x[3], res[3] = 1.25, 1.25          # s = 2.5 everywhere
    _, s, _, _ = check_forward(kind, x, res, gamma, beta, const_row)
    check_backward(kind, dy, s, mean_a, rstd_a, gamma)


@pytest.mark.parametrize("kind,H,rows", FWD_LOOP_CASES)
def test_forward_row_loop_second_trip(dev, lib, kind, H, rows):
    x, res, _, gamma, beta, _, _ = draw(dev, kind, H, rows)
    check_forward(kind, x, res, gamma, beta)
    check_forward(kind, x, None, gamma, beta)          # no residual: the prefetch of the 8-wide kernel has one stream less


@pytest.mark.parametrize("kind,H,rows", BWD_EMPTY_CASES)
def test_backward_blocks_past_the_end_write_zero_records(dev, lib, kind, H, rows):
    x, res, dy, gamma, _, mean_a, rstd_a = draw(dev, kind, H, rows)
    s = (x.float() + res.float()).to(x.dtype)
    part = check_backward(kind, dy, s, mean_a, rstd_a, gamma)
    nb = part.shape[0]
    rpb = -(-rows // nb)
    first_empty = -(-rows // rpb)
    assert (nb, rpb, first_empty) == (768, 5, 616)
    assert bool((part[first_empty:] == 0).all()), "a block without rows must write a zero partial record"
    assert bool((part[:first_empty].abs().amax((1, 2)) > 0).all())


# ------------------------------------------------------------------------------------------------------------------
# dropout masks
# ------------------------------------------------------------------------------------------------------------------
def _rate_ok(keep, p, sixteen_bit, what):
    n = keep.numel()
    expect = round(p * 65536) / 65536 if sixteen_bit else p
    rate = 1.0 - float(keep.double().mean())
    assert abs(rate - expect) <= 5 * math.sqrt(p * (1 - p) / n) + 2.0 ** -16, (what, rate, expect, n)


def _mask_inputs(dev, kind, H, rows, seed):
    x, res, dy, gamma, beta, _, _ = draw(dev, kind, H, rows, seed=seed, beta_mean=0.5)          # beta ~ 0.5: a kept output is never exactly 0
    x[x == 0] = 1.0                                                                             # ... nor a kept input
    return x, res, dy, gamma, beta


def _pre_mask_pair(fwd_off, bwd_off, x, res, dy, gamma, beta, p, rng):
    """forward with p_pre on one form, backward on another -> keep_pre as the forward drew it, and the outputs"""
    _, s0, _, _ = launch_fwd(x, None, gamma, beta, fwd_off, p_pre=p, rng=rng, site=SITE)
    keep = s0 != 0
    y, s, mean, rstd = launch_fwd(x, res, gamma, beta, fwd_off, p_pre=p, rng=rng, site=SITE)
    sr, mr, rr, yr = ln_fwd_ref(x, res, gamma, beta, EPS, keep, None, p, 0.0)
    check_rows(y, yr, D_Y, "y under p_pre")
    check_rows(s, sr, D_DS, "s_out under p_pre")
    check_stats(mean, mr, "mean under p_pre")
    check_stats(rstd, rr, "rstd under p_pre")
    outs = []
    for off in bwd_off:
        ds, dx, part = launch_bwd(dy, s, mean, rstd, gamma, off, p_pre=p, rng=rng, site=SITE)
        dsr, dxr, _, _ = ln_bwd_ref(dy, s, mean, rstd, gamma, keep, None, p, 0.0)
        assert torch.equal(dx != 0, keep), f"dx must be exactly zero where the forward dropped x, and only there ({int(((dx != 0) != keep).sum())} differ)"
        check_rows(ds, dsr, D_DS, "ds under p_pre")
        check_rows(dx, dxr, D_DS, "dx under p_pre")
        check_gamma_beta(part, dy, s, mean, rstd, gamma)
        outs.append((ds, dx))
    return keep, (y, s), outs


def _post_mask_pair(fwd_off, bwd_off, x, res, dy, gamma, beta, p, rng):
    y0, _, _, _ = launch_fwd(x, res, gamma, beta, fwd_off)
    y, s, mean, rstd = launch_fwd(x, res, gamma, beta, fwd_off, p_post=p, rng=rng, site=SITE)
    keep = y != 0
    if y.dtype == torch.float32:          # the kept outputs are the undropped ones times 1 / (1 - p), the factor formed in fp32 as the kernel forms it
        ik = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32))
        assert torch.equal(y[keep], (y0 * ik.to(y.device))[keep])
    _, _, _, yr = ln_fwd_ref(x, res, gamma, beta, EPS, None, keep, 0.0, p)
    check_rows(y, yr, D_Y, "y under p_post")
    outs = []
    for off in bwd_off:
        ds, _, part = launch_bwd(dy, s, mean, rstd, gamma, off, p_post=p, rng=rng, site=SITE)
        dsr, _, _, _ = ln_bwd_ref(dy, s, mean, rstd, gamma, None, keep, 0.0, p)
        check_rows(ds, dsr, D_DS, "ds under p_post")
        got = check_gamma_beta(part, dy, s, mean, rstd, gamma, keep, p)          # dbeta = sum_rows dy keep / (1 - p), per column
        unrelated = dy.double().sum(0) * float(keep.double().mean()) / (1 - p)   # what a mask unrelated to the forward's gives in expectation
        assert rel_l2(got[1], unrelated) > 0.1
        outs.append((ds,))
    return keep, (y, s), outs


@pytest.mark.parametrize("kind,H,p,side", MASK_CASES)
def test_dropout_masks_forward_and_backward(dev, lib, kind, H, p, side):
    from ytvln import ops
    rows = -(-65536 // H) + 3
    off = KINDS[kind][1]
    x, res, dy, gamma, beta = _mask_inputs(dev, kind, H, rows, seed=1)
    rng = ops.DropoutState(dev).tensor
    keep, _, _ = (_pre_mask_pair if side == "pre" else _post_mask_pair)(off, (off,), x, res, dy, gamma, beta, p, rng)
    _rate_ok(keep, p, KINDS[kind][0] and H % 8 == 0, f"{side} drop rate")


@pytest.mark.parametrize("side", ["pre", "post"])
@pytest.mark.parametrize("H", [8, 512, 1024, 2048])
def test_dropout_masks_agree_across_forms_bf16(dev, lib, H, side):
    """(forward 8-wide | 4-wide) x (backward 8-wide | 4-wide) on the same values: one draw scheme (norm.hip 47-59: drop4 with x8 == keep8)."""
    from ytvln import ops
    rows = -(-65536 // H) + 3
    x, res, dy, gamma, beta = _mask_inputs(dev, "bf16x8", H, rows, seed=2)
    rng = ops.DropoutState(dev).tensor
    pair = _pre_mask_pair if side == "pre" else _post_mask_pair
    keep_a, fwd_a, _ = pair(0, (0, OFF), x, res, dy, gamma, beta, 0.25, rng)          # each backward form checks itself against the
    keep_o, fwd_o, _ = pair(OFF, (0, OFF), x, res, dy, gamma, beta, 0.25, rng)       # mask of the forward form it is paired with
    assert torch.equal(keep_a, keep_o), f"the 8-wide and the 4-wide forward drew different masks ({int((keep_a != keep_o).sum())} elements)"
    assert _same_bits(fwd_a[1], fwd_o[1]), "s_out involves no reduction: the two forms must give the same bits"
    _rate_ok(keep_a, 0.25, True, "drop rate")


@pytest.mark.parametrize("side", ["pre", "post"])
@pytest.mark.parametrize("kind,H,rows,trip", [("f32", 32, 16391, 16384), ("bf16x8", 2048, 2055, 2048)])
def test_dropout_masks_beyond_the_grid_cap(dev, lib, kind, H, rows, trip, side):
    """Rows of the forward's second trip: their masks are regenerated by the backward (which walks rows in another order altogether), are drawn
    at the right rate, and are not those of the row the same wave handled one trip earlier."""
    from ytvln import ops
    x, res, dy, gamma, beta = _mask_inputs(dev, kind, H, rows, seed=3)
    rng = ops.DropoutState(dev).tensor
    keep, _, _ = (_pre_mask_pair if side == "pre" else _post_mask_pair)(0, (0,), x, res, dy, gamma, beta, 0.25, rng)
    _rate_ok(keep[trip:], 0.25, kind != "f32", "drop rate past the first trip")
    assert float((keep[trip:] != keep[:rows - trip]).double().mean()) > 0.1


# ------------------------------------------------------------------------------------------------------------------
# embedding forwards: launch_ln with the same NV table
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("H", [36, 260, 516, 1536])
def test_embedding_forwards_per_row(dev, lib, H, precision):
    from ytvln import ops
    import vilbert_ref as O
    N, T, R, V = 3, 7, 7, 29
    g = torch.Generator().manual_seed(H)
    rn = lambda *shape: torch.randn(*shape, generator=g).to(dev)
    S = {"e.word_embeddings.weight": rn(V, H), "e.position_embeddings.weight": rn(T + 2, H), "e.token_type_embeddings.weight": rn(2, H),
         "e.LayerNorm.weight": 1 + 0.1 * rn(H), "e.LayerNorm.bias": 0.1 * rn(H)}
    ids = torch.randint(0, V, (N, T), generator=g).to(dev)
    tt = torch.randint(0, 2, (N, T), generator=g).to(dev)
    P = {"v.image_location_embeddings.weight": rn(H, 5), "v.image_location_embeddings.bias": rn(H),
         "v.image_orientation_embeddings.weight": rn(H, 4), "v.image_orientation_embeddings.bias": rn(H),
         "v.image_next_orientation_embeddings.weight": rn(H, 2), "v.image_next_orientation_embeddings.bias": rn(H),
         "v.image_sequence_embeddings.weight": rn(32, H), "v.LayerNorm.weight": 1 + 0.1 * rn(H), "v.LayerNorm.bias": 0.1 * rn(H)}
    img, loc = rn(N, R, H), rn(N, R, 12)
    loc[..., 11] = torch.randint(0, 32, (N, R), generator=g).float().to(dev)
    bf = precision == "bf16"
    if bf:
        img = img.to(BF)
    ops.set_matmul_precision(precision)
    try:
        yt = ops.text_embed(ids, tt, *S.values())
        yi = ops.image_embed(img, loc, *P.values())
        torch.cuda.synchronize()
    finally:
        ops.set_matmul_precision("fp32")
    assert yt.dtype == yi.dtype == (BF if bf else torch.float32)
    check_rows(yt.reshape(N * T, H), O.text_embeddings({k: v.double() for k, v in S.items()}, ids, tt, pre="e.").reshape(N * T, H), D_Y, "text embedding")
    # the oracle starts at the region features: an identity projection hands it the img rows the kernel was given
    Pd = {k: v.double() for k, v in P.items()}
    Pd["v.image_embeddings.weight"], Pd["v.image_embeddings.bias"] = torch.eye(H, dtype=torch.float64, device=dev), torch.zeros(H, dtype=torch.float64, device=dev)
    check_rows(yi.reshape(N * R, H), O.image_embeddings(Pd, img.double(), loc.double(), pre="v.").reshape(N * R, H), D_Y, "image embedding")


# ------------------------------------------------------------------------------------------------------------------
# both dropouts in one call: one draw, two fully correlated masks -- refused
# ------------------------------------------------------------------------------------------------------------------
def test_both_dropouts_in_one_call_fail_loudly(dev, lib):
    from ytvln import ops, _lib
    rows, H = 64, 256
    x, res, dy, gamma, beta, mean_a, rstd_a = draw(dev, "f32", H, rows)
    st = ops.DropoutState(dev)
    with pytest.raises(RuntimeError, match="both > 0"):
        ops.add_layer_norm(x, res, gamma, beta, 1e-12, 0.25, 0.25, st)
    with pytest.raises(RuntimeError, match="both > 0"):
        ops.AddLayerNormFn.apply(x, res, gamma, beta, 1e-12, 0.25, 0.1, st.tensor, 1)
    with pytest.raises(RuntimeError, match="both > 0"):
        ops.add_layer_norm(x.to(BF), res.to(BF), gamma, beta, 1e-12, 0.25, 0.25, st)
    # through the ABI: a negative status and the library's message, nothing launched (the outputs keep their poison)
    for bf in (False, True):
        sfx, dt = ("bf16", BF) if bf else ("f32", torch.float32)
        xs, out = x.to(dt), [torch.full((rows, H), float("nan"), dtype=dt, device=dev) for _ in range(4)]
        stat = [torch.full((rows,), float("nan"), device=dev) for _ in range(2)]
        part = torch.full((lib.ytvln_ln_bwd_blocks(rows), 2, H), float("nan"), device=dev)
        fwd = lambda pp, pq: getattr(lib, "ytvln_ln_fwd_" + sfx)(xs.data_ptr(), xs.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                                                 stat[0].data_ptr(), stat[1].data_ptr(), rows, H, EPS, pp, pq, st.tensor.data_ptr(), SITE, _stream())
        bwd = lambda pp, pq: getattr(lib, "ytvln_ln_bwd_" + sfx)(xs.data_ptr(), xs.data_ptr(), mean_a.data_ptr(), rstd_a.data_ptr(), gamma.data_ptr(), out[2].data_ptr(),
                                                                 out[3].data_ptr(), *((None,) if bf else ()), part.data_ptr(), rows, H, pp, pq, st.tensor.data_ptr(), SITE, _stream())
        for fn, name in ((fwd, "ln_fwd"), (bwd, "ln_bwd")):
            rc = fn(0.25, 0.25)
            assert rc < 0 and name in lib.ytvln_last_error().decode() and "both > 0" in lib.ytvln_last_error().decode(), (rc, lib.ytvln_last_error())
            assert fn(1e-3, 0.5) < 0
        with pytest.raises(RuntimeError, match="both > 0"):
            _lib.call("ytvln_ln_fwd_" + sfx, xs.data_ptr(), None, gamma.data_ptr(), beta.data_ptr(), out[0].data_ptr(), None, None, None, rows, H, EPS, 0.25, 0.25,
                      st.tensor.data_ptr(), SITE, _stream())
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in out + stat + [part]), "a refused call must not launch anything"
        # each side alone is still accepted
        assert fwd(0.25, 0.0) == 0 and fwd(0.0, 0.25) == 0 and bwd(0.25, 0.0) == 0 and bwd(0.0, 0.25) == 0
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(t).all()) for t in out + stat + [part])
