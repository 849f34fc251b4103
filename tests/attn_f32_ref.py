"""A rounding-aware restatement of the fp32 attention kernels (csrc/attention.hip), shared by tests/test_attn_f32_rows_cpu.py and
tests/test_attn_f32_rows_gpu.py.  Pure torch, CPU or GPU.  Everything that does not depend on the precision -- the exact fp64 reference and its
backward, the score function, the row / block statistics, the masks, the keep-decision recovery, the lazy-reference rule, the bar and the shape
lists -- is tests/attn_bf16_ref.py's, imported, not copied.

`emulate` is the same fp64 mathematics as `attn_bf16_ref.reference(emulate=False)`, rounded to fp32 where the fp32 kernels round and nowhere else
(read from attention.hip; the body names are the kernel's):

  * the contraction q.k is summed in fp32 (mma_rows: 32x32x2 f32 matrix instructions), like every other contraction below;
  * the score goes to fp32 after each of q.k * scale, + mask and + bias (score(): __fmul_rn, __fadd_rn; the bias by a second __fadd_rn) -- at
    -10000 the fp32 grid is 2^-10;
  * the exponent argument s - m_used is an fp32 difference, and __expf is the hardware's base-2 exponential of fp32((s - m) * log2(e)): a
    relative |s - m| * 2^-24 on the probability.  m_used lies in (max - 12, max] (the lazily moved reference, RESCALE_THR), which moves this noise;
  * the running sum l, the rescale factor alpha = __expf(m - m_new) and the products l * alpha, O * alpha are fp32 (attn_fwd_body and its
    d-split / one-wave forms);
  * P * keep * fp32(1 / (1 - p)) is an fp32 product before the P.V contraction, which is summed in fp32 tile by tile (mma_regs_rows);
  * the context is O * fp32(1 / l), stored as fp32;
  * lse = m + logf(l): logf rounded to fp32, the sum rounded to fp32, STORED AS fp32 and read back by every backward body.  At a fully masked pair
    one fp32 step of lse is 2^-10: a relative 1e-3 on every probability of the row;
  * delta = sum dO * O is an fp32 sum over the STORED fp32 context (attn_bwd_dq_body: Cr; attn_bwd_delta_body);
  * the backward bodies recompute p = __expf(s - lse) with the fp32 score and the fp32 lse, by the same base-2 route;
  * dP = dO.V is summed in fp32; dP * keep * fp32(1 / (1 - p)), the difference with delta and the product with p -- dS -- are fp32, and so is
    P * keep / (1 - p) ahead of the dV contraction;
  * dQ = dS.K, dK = dS^T.Q, dV = P~^T.dO are summed in fp32; dq and dk are multiplied by the fp32 scale ON STORE (store_rows), after the sum;
  * fp32 stores.

Not modelled: the ORDER of the fp32 sums inside and between the matrix instructions (torch's float32 matmul has its own), and the last-bit error
of v_exp_f32 / logf themselves.  That order, together with `max_shift`, is the kernel's freedom; tests/test_attn_f32_rows_cpu.py draws it five
independent ways (`permuted`, `max_shift`, `halves`) and holds each draw to the bar.

Two consequences of the fp32 grid at -10000 (2^-10, a relative 1e-3 on a probability) shape the harness; both were found on the reference alone, where
independent orders of the same fp32 sums moved rows of a FULLY MASKED pair by hundreds of times the noise:
  * which grid step a score lands on depends on the last bit of q.k unless q.k is exact -- the fully masked pairs draw q and k on a grid that makes
    it exact in every order (`packed_inputs_f32(grid_pairs=...)`);
  * which grid step lse lands on depends on the last bit of logf(l) -- lse is held to MARGIN x noise + one fp32 step, and the backward of a fully
    masked pair is held to the emulated backward FROM THE STORED lse (`verdict`).

Rows past the end of a ragged query block: the fp32 kernels load zeros for them (load_rowfrag), not the last query as the bf16 kernels do, so their
scores are the bare mask.  `lazy_shift` (written for the bf16 rule) differs from the fp32 kernels there; the rising-maxima construction it is used
on has whole blocks only.
"""
import math

import torch

import attn_bf16_ref as R
from attn_bf16_ref import (BLOCK, INF_KEY, K_OFF, MARGIN, MASKS, OUTPUTS, Q_OFF, RESCALE_THR, SHAPES_BIAS, SHAPES_DROP, SHAPES_EDGES, V_OFF,  # noqa: F401
                           as_dict, heads_of, judge, lazy_shift, lead_length, make_mask, packed_views, recover_keep, row_and_block_errors,
                           scores, with_inf_column, within_bar)

F32 = torch.float32
# (N, heads, d, Tq, Tk): the bf16 lists plus the arms only the fp32 kernels have
SHAPES_EDGES_F32 = SHAPES_EDGES + [
    (2, 2, 12, 33, 65), (2, 2, 48, 33, 65), (2, 2, 96, 65, 33),          # padded heads: DP = 32, 64, 128
    (1, 2, 128, 40, 576),                                                # > 512 keys at a one-wave head size: the multi-wave bodies under default options
    (1, 2, 128, 33, 576),                                                # ... with a ragged second query tile (one two-wave workgroup of 32 + 1 queries)
    (1, 2, 128, 65, 576)]                                                # the ATTN_DSPLIT arm past 512 keys: d > 64 takes two-wave workgroups from two query
#                                                                          tiles on, and the d-split runs in a workgroup left with ONE tile -- an odd number of
#                                                                          tiles >= 3, so 65 queries is the smallest (33 queries are two tiles in one workgroup)
SHAPES_DROP_F32 = SHAPES_DROP + [(2, 3, 96, 65, 33), (1, 2, 128, 40, 576), (2, 2, 64, 100, 37)]          # the last: four query tiles, ragged two-tile key side
ONE_QUERY_SEED = 3          # inputs of (2, 2, 128, 1, 33).  Tq = 1 leaves ONE query row per plane, and with pair 1 fully masked the noise of dv is two scalars: the
#                             fp32 rounding of the two open rows' lse.  With the draw of seed 1 (and 12, of seeds 1 .. 12) the emulation's two happened to be
#                             small and the shifted order came out at 3.07 x noise.  The margin stays 3 and the inputs were redrawn, as for attn_bf16_ref's
#                             DBIAS_SEED; seeds 2 .. 11 all hold the condition at every mask (worst ratio 2.65, seed 3: 1.74).


def edge_seed(shape):
    return ONE_QUERY_SEED if tuple(shape[3:]) == (1, 33) else 1


PAIR_RT = [(72, 20), (20, 72)]          # both swap_problems orders in the forward, dQ and dK/dV launches


def exact(q, k, v, dout, mask, bias, keep, p, scale):
    return R.reference(q, k, v, dout, mask, bias, keep, p, scale, False)


# ---- the fp32 emulation -----------------------------------------------------------------------------------------------------------------------
LOG2E = torch.tensor(math.log2(math.e), dtype=F32)


def exp32(x):
    """__expf on an fp32 tensor: the hardware's 2^t of t = fp32(x * log2(e))"""
    return torch.exp2((x * LOG2E.to(x.device)).double()).to(F32)


def _mm(a, b, halves=False):
    """fp32 matrix product; halves: the contraction (a's last dimension) in two halves added in fp32, as the d-split sums the head dimension"""
    a, b = a.to(F32), b.to(F32)
    if not halves:
        return a @ b
    c = a.shape[-1] // 2
    return a[..., :c] @ b[..., :c, :] + a[..., c:] @ b[..., c:, :]


def scores32(q, k, mask, bias, scale, halves=False):
    """the scores the kernels see (fp64 tensor of fp32 values): q.k summed in fp32, then attn_bf16_ref.scores' three roundings"""
    return scores(q, k, mask, bias, scale, True, qk=_mm(q, k.transpose(-1, -2), halves))


def backward32(q, k, v, dout, s, lse, out, keep, p, scale, halves=False):
    """dq, dk, dv, dS as the fp32 backward bodies compute them from the fp32 scores `s`, the STORED lse and context; keep dense 0/1 or None.
    Separate from `emulate` so that a test can hand the backward other keep decisions, another lse or another context than the forward's."""
    s32, lse32, out32, do32 = s.to(F32), lse.to(F32), out.to(F32), dout.to(F32)
    prob = exp32(s32 - lse32[..., None])
    dP = _mm(dout, v.transpose(-1, -2), halves)
    if halves:
        c = out32.shape[-1] // 2
        delta = ((do32 * out32)[..., :c].sum(-1) + (do32 * out32)[..., c:].sum(-1))[..., None]
    else:
        delta = (do32 * out32).sum(-1, keepdim=True)
    sc = torch.tensor(scale, dtype=F32, device=s.device)
    if keep is None:
        dS, pk = prob * (dP - delta), prob
    else:
        ik = torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32))
        kf = keep.to(F32) * ik.to(s.device)
        dS, pk = prob * (dP * kf - delta), prob * kf
    dq = _mm(dS, k) * sc
    dk = _mm(dS.transpose(-1, -2), q) * sc
    dv = _mm(pk.transpose(-1, -2), dout)
    return dq.double(), dk.double(), dv.double(), dS.double()


def forward32(s, v, keep, p, max_shift=None):
    """out, lse of the fp32 forward bodies from the fp32 scores `s` [N, heads, Tq, Tk]: the online softmax over 32-key tiles with the reference
    m_used = row maximum - max_shift (constant per row and tile; the kernel's rule gives `lazy_shift`'s), l, O and their rescaling in fp32."""
    N, h, Tq, Tk = s.shape
    dev = s.device
    s32 = s.to(F32)
    final = s32.amax(-1)
    final = torch.where(torch.isinf(final), torch.zeros_like(final), final)          # (a row of -inf scores: the kernels take 0 as the reference)
    sh = torch.zeros_like(s32) if max_shift is None else torch.as_tensor(max_shift, device=dev).to(F32).expand(N, h, Tq, Tk)
    v32 = v.to(F32)
    ik = None
    if keep is not None:
        ik = (torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32))).to(dev)
    m = None
    l = torch.zeros(N, h, Tq, dtype=F32, device=dev)
    O = torch.zeros(N, h, Tq, v.shape[-1], dtype=F32, device=dev)
    for j0 in range(0, Tk, BLOCK):
        sl = slice(j0, min(Tk, j0 + BLOCK))
        mn = final - sh[..., j0]
        mn = torch.where(torch.isfinite(mn), mn, torch.zeros_like(mn))
        if m is not None:
            alpha = torch.where(l == 0, torch.ones_like(l), exp32(m - mn))          # (nothing accumulated yet: nothing to rescale)
            l, O = l * alpha, O * alpha[..., None]
        m = mn
        P = exp32(s32[..., sl] - m[..., None])
        l = l + P.sum(-1)
        if keep is not None:
            P = P * ik * keep[..., sl].to(F32)
        O = O + P @ v32[..., sl, :]
    out = O * (1.0 / l)[..., None]
    lse = m + torch.log(l.double()).to(F32)
    return out.double(), lse.double()


def emulate(q, k, v, dout, mask, bias, keep, p, scale, max_shift=None, halves=False):
    """-> out, lse, dq, dk, dv, dS as float64 tensors of fp32 values; arguments as attn_bf16_ref.reference.  halves: every contraction over the
    head dimension (q.k, dO.V, delta) in two halves."""
    s = scores32(q, k, mask, bias, scale, halves)
    out, lse = forward32(s, v, keep, p, max_shift)
    dq, dk, dv, dS = backward32(q, k, v, dout, s, lse, out, keep, p, scale, halves)
    return out, lse, dq, dk, dv, dS


NOISE_SHIFT = RESCALE_THR / 2          # the yardstick emulation exponentiates with m_used = max - 6, the middle of the window the kernel may use


def both(q, k, v, dout, mask, bias, keep, p, scale):
    """(exact, emulated) as dicts (attn_bf16_ref.as_dict).  The emulation whose distance from exact is the NOISE takes max_shift = NOISE_SHIFT: the
    rounding of the exponent argument grows with |s - m_used|, so an emulation at max_shift = 0 understates what a kernel that uses its freedom
    may show (measured on the reference alone, tests/test_attn_f32_rows_cpu.py: shifts drawn in [0, 12) came out at up to 4.4 x the noise of a
    shift-0 emulation, at up to 2.3 x this one's)."""
    return (as_dict(exact(q, k, v, dout, mask, bias, keep, p, scale)),
            as_dict(emulate(q, k, v, dout, mask, bias, keep, p, scale, max_shift=NOISE_SHIFT)))


def reference_base(ref_in, mask, bias, keep, p, scale, full_pairs=()):
    """what `verdict` needs of the reference alone: (exact, emulated, noise_from); computed once per case and shared between the kernel forms"""
    q, k, v, dout = ref_in
    noise_from = None
    if len(full_pairs) == q.shape[0]:          # no open pair: the noise of the same inputs without a mask
        noise_from = both(q, k, v, dout, None, bias, keep, p, scale)
    return both(q, k, v, dout, mask, bias, keep, p, scale) + (noise_from,)


def verdict(got, got_lse, ref_in, mask, bias, keep, p, scale, full_pairs=(), base=None):
    """The bar of the fp32 row tests.  got: dict name -> [N, heads, T, d] (any of OUTPUTS), got_lse [N, heads, Tq] the log-sum-exp that came with it,
    ref_in = (q, k, v, dout) float64 views.  `attn_bf16_ref.judge` with one addition for the fully masked pairs `full_pairs`: there lse is about
    -10000, ONE fp32 step of it (2^-10) is a relative 1e-3 on every probability of the row, and which of two neighbouring steps fp32(m + logf(l))
    lands on is decided by the last bit of logf(l) -- the order of l's sum, the reference m the kernel holds.  So lse is held per row to
    MARGIN x noise + one fp32 step (`judge_lse`), and the emulated yardstick of a fully masked pair's dq / dk / dv is `backward32` FROM THE lse
    THAT WAS STORED (`got_lse`): the backward bodies are held to exponentiating against exactly what the forward stored, to the step.
    base: `reference_base` of the same arguments where the caller has it.
    -> (res as `judge` gives it, lse_res as `judge_lse` gives it, exact, emul)"""
    q, k, v, dout = ref_in
    ex, em, noise_from = base if base is not None else reference_base(ref_in, mask, bias, keep, p, scale, full_pairs)
    if full_pairs:
        em = {n: t.clone() for n, t in em.items()}          # (`base` may be shared between callers: left unchanged)
        s = scores32(q, k, mask, bias, scale)
        for n in full_pairs:
            one = slice(n, n + 1)
            dq, dk, dv, _ = backward32(q[one], k[one], v[one], dout[one], s[one], got_lse[one].double(), em["out"][one],
                                       None if keep is None else keep[one], p, scale)
            em["dq"][one], em["dk"][one], em["dv"][one] = dq, dk, dv
    res = judge(got, ex, em, full_pairs, noise_from)
    lse_res = judge_lse(got_lse, ex["lse"], em["lse"], full_pairs, None if noise_from is None else (noise_from[0]["lse"], noise_from[1]["lse"]))
    return res, lse_res, ex, em


def permuted(fn, q, k, v, dout, mask, bias, keep, qperm, kperm):
    """fn(q, k, v, dout, mask, bias, keep) -> (out, lse, dq, dk, dv, dS) evaluated with the queries in order `qperm` and the keys in order `kperm`
    (index tensors), results put back in the original order: the same mathematics with every sum over keys or queries taken in another order."""
    iq, ikk = torch.argsort(qperm), torch.argsort(kperm)
    out, lse, dq, dk, dv, dS = fn(q[:, :, qperm], k[:, :, kperm], v[:, :, kperm], dout[:, :, qperm], None if mask is None else mask[:, kperm],
                                  None if bias is None else bias[:, :, qperm][:, :, :, kperm], None if keep is None else keep[:, :, qperm][:, :, :, kperm])
    return out[:, :, iq], lse[:, :, iq], dq[:, :, iq], dk[:, :, ikk], dv[:, :, ikk], dS[:, :, iq][:, :, :, ikk]


def tile_permutation(T, seed):
    """0 .. T-1 with its 32-element tiles in a random order (the ragged last tile moves with the others)"""
    tiles = list(torch.arange(T).split(BLOCK))
    order = torch.randperm(len(tiles), generator=torch.Generator().manual_seed(seed)).tolist()
    return torch.cat([tiles[i] for i in order])


def block_tile_shift(N, heads, Tq, Tk, seed):
    """a max_shift drawn U[0, 12) per (query block, key tile), expanded to the scores"""
    nb, nt = -(-Tq // BLOCK), -(-Tk // BLOCK)
    u = torch.rand((N, heads, nb, nt), generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * RESCALE_THR
    return u.repeat_interleave(BLOCK, 2).repeat_interleave(BLOCK, 3)[:, :, :Tq, :Tk]


# ---- lse and probabilities per row ---------------------------------------------------------------------------------------------------------------
def f32_step(x):
    """one fp32 step at |x| (fp64 tensor)"""
    x32 = x.abs().to(F32)
    return (torch.nextafter(x32, torch.full_like(x32, float("inf"))) - x32).double()


def judge_lse(got, exact_lse, emul_lse, full_pairs=(), noise_from=None):
    """lse [N, heads, Tq] per row: open pairs against exact fp64, fully masked pairs against the emulated value; the bound of a row is
    MARGIN x noise + one fp32 step of |lse|, noise = the largest |emulated - exact| over the open pairs (of `noise_from` = (exact, emulated) lse of
    the same inputs without a mask when there is no open pair).  -> dict(err, noise, worst = largest err / bound)"""
    N = exact_lse.shape[0]
    open_pairs = [n for n in range(N) if n not in full_pairs]
    yard = exact_lse.clone()
    for n in full_pairs:
        yard[n] = emul_lse[n]
    noise = float((emul_lse[open_pairs] - exact_lse[open_pairs]).abs().max()) if open_pairs else float((noise_from[1] - noise_from[0]).abs().max())
    err = (got.double() - yard).abs()
    bound = MARGIN * noise + f32_step(yard)
    return dict(err=float(err.max()), noise=noise, worst=float((err / bound).max()))


def probs_of(s, lse, emulated):
    """exp(s - lse) [N, heads, Tq, Tk]: exact fp64, or as attn_probs_body computes it from fp32 scores and the fp32 lse"""
    if not emulated:
        return torch.exp(s - lse[..., None])
    return exp32(s.to(F32) - lse.to(F32)[..., None]).double()


# ---- inputs: drawn on the CPU in fp32 so that the CPU and the GPU tests judge the same tensors ------------------------------------------------------
GRID = 2.0 ** -6


def packed_inputs_f32(N, heads, d, Tq, Tk, seed=1, grid_pairs=()):
    """attn_bf16_ref.packed_inputs in fp32: A [N*Tq, 3H], B [N*Tk, 3H], dout [N*Tq, H]; q in column block 2 of A, k | v in blocks 1 | 2 of B.
    grid_pairs: pairs whose q and k are rounded to multiples of 2^-6 (|x| < 4: 8 bits).  Their products are multiples of 2^-12 below 16 and a sum
    of up to 128 of them has at most 23 bits, so q.k is EXACT in fp32 in every order of summation.  For the fully masked pairs: there the score
    fp32(fp32(q.k * scale) - 10000) lies on a grid of 2^-10, a step of which is a relative 1e-3 on a probability; with an inexact q.k the step a
    score lands on would depend on the last bit of the sum, i.e. on its order (summing q.k in two halves of d moved rows of such a pair by
    150 .. 700 x noise).  With an exact q.k every form of the kernel and the emulation must agree on every score of the pair to the bit, and
    one wrong grid step is a defect, not a rounding."""
    A, B, dout = R.packed_inputs(N, heads, d, Tq, Tk, seed, dtype=F32)
    H = heads * d
    for n in grid_pairs:
        for X, T, off in ((A, Tq, Q_OFF), (B, Tk, K_OFF)):
            blk = X[n * T:(n + 1) * T, off * H:(off + 1) * H]
            blk.copy_(torch.round(blk / GRID).clamp(-255, 255) * GRID)
    return A, B, dout


def rising_inputs_f32(d, N=2, heads=2, Tq=64, Tk=160, seed=5):
    """attn_bf16_ref.rising_inputs without the bf16 rounding"""
    return R.rising_inputs(d, N, heads, Tq, Tk, seed, dtype=F32)


def pair_inputs_f32(N, Rr, T, heads, d, seed=11):
    return R.pair_inputs(N, Rr, T, heads, d, seed, dtype=F32)
