"""CPU: the harness of tests/test_attn_bf16_blocks_gpu.py judged from the reference alone (tests/attn_bf16_ref.py).

The GPU tests hold the bf16 attention kernels, per row and per 32-row block, to 3 x noise, where noise = the rounding-aware fp64 emulation of the
kernels against exact fp64 on the same inputs.  That bar is legitimate only if an INDEPENDENT draw of what the kernel is free to do -- its lazily
moved softmax reference, i.e. other rounding decisions for every probability -- stays under it (the noise condition, on the very inputs the GPU
tests use), and it is worth something only if defects of one row, one tile or one mask word exceed it by a wide factor while the whole-tensor
relative L2 the older tests assert (2e-2) lets them pass (the planted faults).  The keep-mask decoder is checked against a packer written from the
layout comment of attention_bf16.hip."""
import math

import pytest
import torch

import attn_bf16_ref as R
from helpers import rel_l2
from test_attn_bias_gpu import make_bias          # (an input builder; nothing of that module runs here)

SEEDS = 10
P_DROP = 0.1


def _keep(shape, p, seed):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) >= p).double()


def _both(q, k, v, do, mask, bias, keep, p, scale):
    return (R.as_dict(R.reference(q, k, v, do, mask, bias, keep, p, scale, False)),
            R.as_dict(R.reference(q, k, v, do, mask, bias, keep, p, scale, True)))


def _noise_condition(q, k, v, do, mask, bias, keep, p, scale, full_pairs=(), shifts=None, what="", check_ds=False):
    """3 x noise holds for `SEEDS` independent draws of the per-row shift U[0, 12) (or for the given shifts); -> the worst ratio seen"""
    exact, emul = _both(q, k, v, do, mask, bias, keep, p, scale)
    noise_from = None
    if len(full_pairs) == q.shape[0]:          # no open pair: the noise of the same inputs without a mask
        noise_from = _both(q, k, v, do, None, bias, keep, p, scale)
    N, h, Tq, _ = q.shape
    worst = 0.0
    for sd in range(SEEDS if shifts is None else len(shifts)):
        sh = torch.rand((N, h, Tq, 1), generator=torch.Generator().manual_seed(100 + sd), dtype=torch.float64) * 12 if shifts is None else shifts[sd]
        other = R.as_dict(R.reference(q, k, v, do, mask, bias, keep, p, scale, True, max_shift=sh))
        res = R.judge({n: other[n] for n in R.OUTPUTS}, exact, emul, full_pairs, noise_from)
        for name, r in res.items():
            assert r["noise_row"] > 0 and r["noise_blk"] > 0, (what, name)
            worst = max(worst, r["row"] / r["noise_row"], r["blk"] / r["noise_blk"])
            assert R.within_bar({name: r}), (what, sd, name, r)
        if check_ds:          # the bias gradient's yardstick: dS before its rounding, per 32-query block
            _, blk, _ = R.row_and_block_errors(other["dS"], exact["dS"])
            _, nblk, _ = R.row_and_block_errors(emul["dS"], exact["dS"])
            worst = max(worst, float(blk.max()) / float(nblk.max()))
            assert float(blk.max()) <= R.MARGIN * float(nblk.max()), (what, sd, "dS", float(blk.max()), float(nblk.max()))
    return worst


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("pattern", R.MASKS)
@pytest.mark.parametrize("N,heads,d,Tq,Tk", R.SHAPES_EDGES)
def test_noise_condition_granule_edges(N, heads, d, Tq, Tk, pattern, drop):
    A, B, dout = R.packed_inputs(N, heads, d, Tq, Tk)
    q, k, v, do = R.packed_views(A, B, dout, N, heads, d, Tq, Tk)
    mask = R.make_mask(N, Tk, pattern)
    keep = _keep((N, heads, Tq, Tk), P_DROP, 3) if drop else None
    full = (N - 1,) if pattern == "full" else ()
    w = _noise_condition(q, k, v, do, mask, None, keep, P_DROP if drop else 0.0, 1 / math.sqrt(d), full, what=(N, heads, d, Tq, Tk, pattern, drop))
    print(f"noise condition edges {(N, heads, d, Tq, Tk)} {pattern} drop {drop}: worst ratio {w:.2f}")


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("N,heads,d,Tq,Tk", R.SHAPES_DROP)
def test_noise_condition_dropout_shapes(N, heads, d, Tq, Tk, p):
    A, B, dout = R.packed_inputs(N, heads, d, Tq, Tk)
    q, k, v, do = R.packed_views(A, B, dout, N, heads, d, Tq, Tk)
    keep = _keep((N, heads, Tq, Tk), p, 4) if p > 0 else None
    _noise_condition(q, k, v, do, R.make_mask(N, Tk, "tail"), None, keep, p, 1 / math.sqrt(d), what=(N, heads, d, Tq, Tk, p))


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("side", [None, 1])
@pytest.mark.parametrize("d", [64, 128])
def test_noise_condition_pair_launch(d, side, drop):
    N, Rr, T, heads = 2, 70, 45, 2
    q1, kv1, q2, kv2, m1, m2, g1, g2 = R.pair_inputs(N, Rr, T, heads, d)
    Hb = heads * d
    p = P_DROP if drop else 0.0
    bias1 = make_bias("cpu", "n1", N, heads, Rr, T, seed=21)[1].transpose(2, 3) if side == 1 else None          # (the co-attention mask's transposed view)
    for (q, kv, g, mask, Tq, Tk, bias) in ((q2, kv1, g1, m1, T, Rr, bias1), (q1, kv2, g2, m2, Rr, T, None)):
        qq, kk, vv, do = (R.heads_of(x, N, t, heads, d) for x, t in ((q, Tq), (kv[:, :Hb], Tk), (kv[:, Hb:], Tk), (g, Tq)))
        keep = _keep((N, heads, Tq, Tk), p, 5) if drop else None
        _noise_condition(qq, kk, vv, do, mask, bias, keep, p, 1 / math.sqrt(d), what=(d, side, drop, Tq, Tk))


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("form", ["nh", "n1T"])
@pytest.mark.parametrize("N,heads,d,Tq,Tk", R.SHAPES_BIAS)
def test_noise_condition_bias_forms(N, heads, d, Tq, Tk, form, drop):
    A, B, dout = R.packed_inputs(N, heads, d, Tq, Tk)
    q, k, v, do = R.packed_views(A, B, dout, N, heads, d, Tq, Tk)
    bias = R.with_inf_column(make_bias("cpu", form, N, heads, Tq, Tk)[0]).double().expand(N, heads, Tq, Tk)
    keep = _keep((N, heads, Tq, Tk), P_DROP, 6) if drop else None
    _noise_condition(q, k, v, do, R.make_mask(N, Tk, "tail"), bias, keep, P_DROP if drop else 0.0, 1 / math.sqrt(d), what=(N, heads, d, Tq, Tk, form))


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("N,heads,d,Tq,Tk", R.SHAPES_DBIAS)
def test_noise_condition_bias_gradient(N, heads, d, Tq, Tk, drop):
    """the bias gradient's yardstick is dS before its rounding, per 32-query block (inputs: see attn_bf16_ref.DBIAS_SEED)"""
    A, B, dout = R.packed_inputs(N, heads, d, Tq, Tk, seed=R.DBIAS_SEED)
    q, k, v, do = R.packed_views(A, B, dout, N, heads, d, Tq, Tk)
    bias = make_bias("cpu", "nh", N, heads, Tq, Tk)[1]
    keep = _keep((N, heads, Tq, Tk), P_DROP, 6) if drop else None
    w = _noise_condition(q, k, v, do, R.make_mask(N, Tk, "tail"), bias, keep, P_DROP if drop else 0.0, 1 / math.sqrt(d), what=(N, heads, d, Tq, Tk),
                         check_ds=True)
    print(f"noise condition bias gradient {(N, heads, d, Tq, Tk)} drop {drop}: worst ratio {w:.2f}")


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_noise_condition_rising_maxima_with_the_true_staleness(d, drop):
    """Here the kernel's softmax reference really is stale: the shift is what the kernel's own rule gives for these scores (`lazy_shift`), and the
    construction is checked to contain, inside ONE 32-query block, tiles at which the reference moves after the first, stale rows where it does
    not, and rows whose maximum lies in the first tile."""
    N, heads, Tq, Tk = 2, 2, 64, 160
    q2, k2, v2, do2 = R.rising_inputs(d)
    q, k, v, do = (R.heads_of(x, N, t, heads, d) for x, t in ((q2, Tq), (k2, Tk), (v2, Tk), (do2, Tq)))
    scale = 1 / math.sqrt(d)
    s = R.scores(q, k, None, None, scale, True)
    shift, stale, moved = R.lazy_shift(s)
    assert float(stale.min()) >= 0 and float(stale.max()) <= R.RESCALE_THR
    b0 = moved[0, 0, 0]          # query block 0 of plane (0, 0)
    assert bool(b0[0]) and bool(b0[1:].any()) and not bool(b0[1:].all()), b0
    still = [t for t in range(1, 5) if not bool(b0[t])]
    assert float(stale[0, 0, :32, still[0] * 32:(still[0] + 1) * 32].max()) > 3, "rows of the block are stale where the wave did not move"
    assert bool((s[0, 0, :32].argmax(-1) < 32).any()) and bool((s[0, 0, :32].argmax(-1) >= 128).any()), "rows that go down, rows that climb"
    assert not bool(moved[0, 0, 1, 1:].any()) and float(stale[0, 0, 32:].max()) > 3, "query block 1 never moves after the first tile"
    keep = _keep((N, heads, Tq, Tk), P_DROP, 7) if drop else None
    w = _noise_condition(q, k, v, do, None, None, keep, P_DROP if drop else 0.0, scale, shifts=[shift], what=("rising", d, drop))
    print(f"noise condition rising maxima d {d} drop {drop}: worst ratio {w:.2f}")


# ---- planted faults ---------------------------------------------------------------------------------------------------------------------------
FACTOR = 5.0


def _big_case():
    N, heads, d, Tq, Tk = 2, 8, 128, 80, 288
    A, B, dout = R.packed_inputs(N, heads, d, Tq, Tk)
    q, k, v, do = R.packed_views(A, B, dout, N, heads, d, Tq, Tk)
    mask = R.make_mask(N, Tk, "tail")
    keep = _keep((N, heads, Tq, Tk), P_DROP, 8)
    scale = 1 / math.sqrt(d)
    exact, emul = _both(q, k, v, do, mask, None, keep, P_DROP, scale)
    noise = {n: float(R.row_and_block_errors(emul[n], exact[n])[0].max()) for n in R.OUTPUTS}
    s = R.scores(q, k, mask, None, scale, True)
    return dict(q=q, k=k, v=v, do=do, keep=keep, scale=scale, exact=exact, emul=emul, noise=noise, s=s, kf=keep / (1 - P_DROP))


@pytest.fixture(scope="module")
def big():
    return _big_case()


def _caught(name, faulty, c, what):
    """the per-row statistic of the faulty tensor exceeds 3 x noise by FACTOR while its whole-tensor relative L2 passes the old 2e-2"""
    row = float(R.row_and_block_errors(faulty, c["exact"][name])[0].max())
    whole = rel_l2(faulty, c["exact"][name])
    print(f"planted fault {what}: {name} worst row {row:.3f} = {row / c['noise'][name]:.0f} x noise {c['noise'][name]:.2e}, whole-tensor rel l2 {whole:.2e}")
    assert row > FACTOR * R.MARGIN * c["noise"][name], (what, name, row, c["noise"][name])
    assert whole < 2e-2, (what, name, whole)
    assert rel_l2(c["emul"][name], c["exact"][name]) < whole, "the fault is visible in the whole-tensor figure, just not over its bar"


def test_fault_one_query_row_loses_one_key_tile_of_ds(big):
    """dS[pair 1, head 3, query 17, keys 128..159] never reaches the dQ contraction: one wrong row of dq in 1280"""
    c = big
    dSb = R.bf16_round(c["emul"]["dS"]).clone()
    dSb[1, 3, 17, 128:160] = 0
    _caught("dq", R.bf16_round(dSb @ c["k"] * c["scale"]), c, "a (dS tile lost for one query)")


def test_fault_one_key_row_of_p_zeroed_in_the_dv_contraction(big):
    c = big
    prob = torch.exp(c["s"] - c["emul"]["lse"][..., None])
    pk = R.bf16_round(prob * c["kf"]).clone()
    pk[0, 5, :, 77] = 0
    _caught("dv", R.bf16_round(pk.transpose(-1, -2) @ c["do"]), c, "b (one key of P zeroed for dV)")


def test_fault_one_keep_word_from_the_neighbouring_key_tile(big):
    """The dK/dV kernel reads mask word r = 6 of (query block 1, key tile 3) from key tile 4: 64 decisions, the keys bkrow(6, 0) and bkrow(6, 1)
    of the tile for 32 queries.  The forward (context, lse, delta) used the right decisions."""
    c = big
    keep = c["keep"].clone()
    for half in range(2):
        j = R.bkrow(6, half)
        keep[1, 2, 32:64, 3 * 32 + j] = c["keep"][1, 2, 32:64, 4 * 32 + j]
    assert int((keep != c["keep"]).sum()) > 4
    _, dk, dv, _ = R.backward_from(c["q"], c["k"], c["v"], c["do"], c["s"], c["emul"]["lse"], c["emul"]["out"], keep / (1 - P_DROP), c["scale"], True)
    _caught("dv", dv, c, "c (keep word of the neighbouring tile, dV)")


def test_fault_ragged_last_key_tile_read_with_its_clamped_rows_unmasked():
    """Tk = 101: the LDS-DMA clamps rows 101..127 of the last key tile to key 100, and the forward gives them a mask of -inf.  The fault: one
    wave -- the 32 queries of block 1 of plane (pair 0, head 2) -- gives them the mask of the row they were clamped to instead, so 27 copies of
    key 100 take part in that block's softmax.  The last key is a soft-masked one (mask -3.25: it carries weight e^-3.25 of an open key), which is
    what keeps the damage of 32 rows in 2304 below the whole-tensor bar; with an open last key the same fault is far over every bar."""
    N, heads, d, Tq, Tk = 2, 4, 64, 288, 101
    A, B, dout = R.packed_inputs(N, heads, d, Tq, Tk)
    q, k, v, do = R.packed_views(A, B, dout, N, heads, d, Tq, Tk)
    mask = torch.zeros(N, Tk)
    mask[:, Tk - 1] = -3.25
    scale = 1 / math.sqrt(d)
    exact, emul = _both(q, k, v, do, mask, None, None, 0.0, scale)
    c = dict(exact=exact, emul=emul, noise={n: float(R.row_and_block_errors(emul[n], exact[n])[0].max()) for n in R.OUTPUTS})
    n, h, rows = 0, 2, slice(32, 64)
    ext = lambda x: torch.cat([x[n:n + 1, h:h + 1], x[n:n + 1, h:h + 1, Tk - 1:].expand(1, 1, 128 - Tk, d)], 2)          # noqa: E731
    mext = torch.cat([mask[n:n + 1], mask[n:n + 1, Tk - 1:].expand(1, 128 - Tk)], 1)
    bad = R.as_dict(R.reference(q[n:n + 1, h:h + 1, rows], ext(k), ext(v), do[n:n + 1, h:h + 1, rows], mext, None, None, 0.0, scale, True))
    for name in ("out", "dq"):
        faulty = emul[name].clone()
        faulty[n, h, rows] = bad[name][0, 0]
        _caught(name, faulty, c, "d (clamped rows of the ragged key tile unmasked)")


# ---- keep-mask layout -------------------------------------------------------------------------------------------------------------------------
def _pack_keep(dense, fill):
    """Written from the header of attention_bf16.hip: for accumulator register r of a (32 queries x 32 keys) block a 64-bit lane mask, lane =
    query + 32 half, key = bkrow(r, half) = (r & 3) + 8 (r >> 2) + 4 half; 16 masks per block, [pair * head][query block][key tile][16].
    `fill` [.., 32 nb, 32 nt] supplies the bits of queries / keys past the end."""
    N, heads, Tq, Tk = dense.shape
    nb, nt = -(-Tq // 32), -(-Tk // 32)
    full = fill.clone()
    full[:, :, :Tq, :Tk] = dense
    words = torch.zeros(N * heads, nb, nt, 16, dtype=torch.int64)
    for ph in range(N * heads):
        plane = full[ph // heads, ph % heads]
        for b in range(nb):
            for t in range(nt):
                for r in range(16):
                    w = 0
                    for lane in range(64):
                        query, half = lane & 31, lane >> 5
                        key = (r & 3) + 8 * (r >> 2) + 4 * half
                        w |= int(plane[32 * b + query, 32 * t + key]) << lane
                    words[ph, b, t, r] = w - (1 << 64) if w >= (1 << 63) else w
    return words.view(-1).view(torch.uint8)


def test_decode_keep_inverts_the_documented_layout():
    N, heads, Tq, Tk = 1, 2, 37, 101
    g = torch.Generator().manual_seed(0)
    dense = (torch.rand((N, heads, Tq, Tk), generator=g) < 0.6).long()
    for fill_value in (0, 1, None):          # whatever the bits past the end hold, they are ignored
        fill = (torch.rand((N, heads, 64, 128), generator=g) < 0.5).long() if fill_value is None else torch.full((N, heads, 64, 128), fill_value)
        buf = _pack_keep(dense, fill)
        assert buf.numel() == N * heads * 2 * 4 * 128
        assert torch.equal(R.decode_keep(buf, N, heads, Tq, Tk), dense.double())


def test_row_and_block_errors_on_a_hand_made_case():
    """one wrong row of norm-1 error in a block whose rows have norm 2: row statistic 1/2, block statistic 1 / sqrt(32 * 4); a ragged second
    block of 5 rows that is identically zero is flagged, not dropped"""
    ref = torch.zeros(1, 1, 37, 4, dtype=torch.float64)
    ref[0, 0, :32, 0] = 2.0
    got = ref.clone()
    got[0, 0, 3, 1] = 1.0
    row, blk, zero = R.row_and_block_errors(got, ref)
    assert row.shape == (1, 1, 37) and blk.shape == (1, 1, 2) and zero.tolist() == [[[False, True]]]
    assert float(row[0, 0, 3]) == 0.5 and float(row.sum()) == 0.5
    assert abs(float(blk[0, 0, 0]) - 1 / math.sqrt(128)) < 1e-15 and float(blk[0, 0, 1]) == 0
    # a tiny row inside a block of large rows is judged against the block's rms row norm, not its own
    ref[0, 0, 7, 0] = 1e-6
    row, _, _ = R.row_and_block_errors(ref * 1.001, ref)
    assert float(row[0, 0, 7]) < 1e-8 and abs(float(row[0, 0, 0]) - 1e-3) < 1e-9
