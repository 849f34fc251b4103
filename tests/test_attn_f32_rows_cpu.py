"""CPU: the harness of tests/test_attn_f32_rows_gpu.py judged from the reference alone (tests/attn_f32_ref.py).

The GPU tests hold the fp32 attention kernels (csrc/attention.hip), per row and per 32-row block and under every kernel form, to MARGIN = 3 x noise,
where noise = the fp32 emulation of the kernels against exact fp64 on the same inputs.  That bar is legitimate only if INDEPENDENT fp32
evaluations of the same mathematics stay under it on the very inputs the GPU tests run.  Five are drawn for every case:
  reversed  every sum over keys and over queries taken in the reversed order;
  tiles     the 32-key and 32-query tiles in a permuted order;
  lazy      the online softmax with the staleness the kernel's own rule gives (`lazy_shift`);
  random    a softmax reference stale by U[0, 12) per (query block, key tile);
  halves    every contraction over the head dimension in two halves, as the d-split form sums it.
The largest ratio these draws show over all cases of this file is 2.67 (at 64 x 1000, fully masked; 2.3 on the open granule-edge cases; every
case prints its own and asserts the bar), so the project's MARGIN = 3 stands; no margin of its own was needed.  What was needed is written in attn_f32_ref's docstring: the yardstick emulation sits in the middle of the kernel's
window of softmax references, and the fully masked pairs take inputs whose q.k is exact and a backward yardstick from the stored lse.

And the bar is worth something only if defects of one row, one tile, one keep decision or one grid step exceed it while the whole-tensor relative
L2 the older tests assert (2e-5) lets them pass where the fault is small enough (the planted faults)."""
import math

import pytest
import torch

import attn_f32_ref as F
from helpers import rel_l2
from test_attn_bias_gpu import make_bias          # (an input builder; nothing of that module runs here)

P_DROP = 0.1
OLD_BAR = 2e-5          # test_attention_fwd_bwd / test_attention_dropout: rel_l2 over the whole tensor


def _keep(shape, p, seed):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) >= p).double()


def _orders(ref_in, mask, bias, keep, p, scale, lazy=None):
    q, k, v, do = ref_in
    N, h, Tq, _ = q.shape
    Tk = k.shape[2]

    def em(**kw):
        return lambda q_, k_, v_, do_, mask_, bias_, keep_: F.emulate(q_, k_, v_, do_, mask_, bias_, keep_, p, scale, **kw)
    yield "reversed", F.permuted(em(), q, k, v, do, mask, bias, keep, torch.arange(Tq).flip(0), torch.arange(Tk).flip(0))
    yield "tiles", F.permuted(em(), q, k, v, do, mask, bias, keep, F.tile_permutation(Tq, 1), F.tile_permutation(Tk, 2))
    if lazy is None:
        lazy = F.lazy_shift(F.scores32(q, k, mask, bias, scale))[0]
    yield "lazy", F.emulate(q, k, v, do, mask, bias, keep, p, scale, max_shift=lazy)
    yield "random", F.emulate(q, k, v, do, mask, bias, keep, p, scale, max_shift=F.block_tile_shift(N, h, Tq, Tk, 3))
    yield "halves", F.emulate(q, k, v, do, mask, bias, keep, p, scale, halves=True)


def _noise_condition(ref_in, mask, bias, keep, p, scale, full_pairs=(), what="", lazy=None):
    """every one of the five orders within MARGIN x noise per row and per block, its lse within the lse bound; -> the worst ratio seen"""
    worst = 0.0
    for order, o in _orders(ref_in, mask, bias, keep, p, scale, lazy):
        o = F.as_dict(o)
        res, lres, _, _ = F.verdict({n: o[n] for n in F.OUTPUTS}, o["lse"], ref_in, mask, bias, keep, p, scale, full_pairs)
        for name, r in res.items():
            assert r["noise_row"] > 0 and r["noise_blk"] > 0, (what, name)
            worst = max(worst, r["row"] / r["noise_row"], r["blk"] / r["noise_blk"])
            assert F.within_bar({name: r}), (what, order, name, r)
        assert lres["worst"] <= 1.0, (what, order, "lse", lres)
    print(f"noise condition {what}: worst ratio {worst:.2f}")
    return worst


@pytest.mark.parametrize("pattern", F.MASKS)
@pytest.mark.parametrize("N,heads,d,Tq,Tk", F.SHAPES_EDGES_F32)
def test_noise_condition_granule_edges(N, heads, d, Tq, Tk, pattern):
    full = (N - 1,) if pattern == "full" else ()
    A, B, dout = F.packed_inputs_f32(N, heads, d, Tq, Tk, seed=F.edge_seed((N, heads, d, Tq, Tk)), grid_pairs=full)
    ref_in = F.packed_views(A, B, dout, N, heads, d, Tq, Tk)
    _noise_condition(ref_in, F.make_mask(N, Tk, pattern), None, None, 0.0, 1 / math.sqrt(d), full, what=("edges", N, heads, d, Tq, Tk, pattern))


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("N,heads,d,Tq,Tk", F.SHAPES_DROP_F32)
def test_noise_condition_dropout_shapes(N, heads, d, Tq, Tk, p):
    A, B, dout = F.packed_inputs_f32(N, heads, d, Tq, Tk)
    ref_in = F.packed_views(A, B, dout, N, heads, d, Tq, Tk)
    _noise_condition(ref_in, F.make_mask(N, Tk, "tail"), None, _keep((N, heads, Tq, Tk), p, 4), p, 1 / math.sqrt(d), what=("drop", N, heads, d, Tq, Tk, p))


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("Rr,T", F.PAIR_RT)
def test_noise_condition_pair_launch(Rr, T, d, p):
    N, heads = 2, 2
    q1, kv1, q2, kv2, m1, m2, g1, g2 = F.pair_inputs_f32(N, Rr, T, heads, d)
    Hb = heads * d
    for (q, kv, g, mask, Tq, Tk) in ((q2, kv1, g1, m1, T, Rr), (q1, kv2, g2, m2, Rr, T)):
        ref_in = tuple(F.heads_of(x, N, t, heads, d) for x, t in ((q, Tq), (kv[:, :Hb], Tk), (kv[:, Hb:], Tk), (g, Tq)))
        keep = _keep((N, heads, Tq, Tk), p, 5) if p > 0 else None
        _noise_condition(ref_in, mask, None, keep, p, 1 / math.sqrt(d), what=("pair", Rr, T, d, p, Tq, Tk))


@pytest.mark.parametrize("form", ["nh", "n1T"])
@pytest.mark.parametrize("N,heads,d,Tq,Tk", F.SHAPES_BIAS)
def test_noise_condition_bias_forms(N, heads, d, Tq, Tk, form):
    A, B, dout = F.packed_inputs_f32(N, heads, d, Tq, Tk)
    ref_in = F.packed_views(A, B, dout, N, heads, d, Tq, Tk)
    bias = F.with_inf_column(make_bias("cpu", form, N, heads, Tq, Tk)[0]).double().expand(N, heads, Tq, Tk)
    _noise_condition(ref_in, F.make_mask(N, Tk, "tail"), bias, None, 0.0, 1 / math.sqrt(d), what=("bias", N, heads, d, Tq, Tk, form))


@pytest.mark.parametrize("d", [64, 128])
def test_rising_maxima_take_both_branches_and_hold_the_noise_condition(d):
    """The kernel's softmax reference really is stale here: the construction is checked to contain, inside ONE 32-query block, tiles at which the
    reference moves after the first, stale rows (by more than 3) where it does not, and rows whose maximum lies in the first tile -- on the fp32
    inputs, without the bf16 rounding the construction was first made with."""
    N, heads, Tq, Tk = 2, 2, 64, 160
    q2, k2, v2, do2 = F.rising_inputs_f32(d)
    assert all(t.dtype == torch.float32 for t in (q2, k2, v2, do2))
    ref_in = tuple(F.heads_of(x, N, t, heads, d) for x, t in ((q2, Tq), (k2, Tk), (v2, Tk), (do2, Tq)))
    scale = 1 / math.sqrt(d)
    s = F.scores32(ref_in[0], ref_in[1], None, None, scale)
    shift, stale, moved = F.lazy_shift(s)
    assert float(stale.min()) >= 0 and float(stale.max()) <= F.RESCALE_THR
    b0 = moved[0, 0, 0]          # query block 0 of plane (0, 0)
    assert bool(b0[1:].any()) and not bool(b0[1:].all()) and float(stale[0, 0, :32].max()) > 3, "the construction takes both branches in one block"
    assert bool(b0[0]), b0
    still = [t for t in range(1, 5) if not bool(b0[t])]
    assert float(stale[0, 0, :32, still[0] * 32:(still[0] + 1) * 32].max()) > 3, "rows of the block are stale where the wave did not move"
    assert bool((s[0, 0, :32].argmax(-1) < 32).any()) and bool((s[0, 0, :32].argmax(-1) >= 128).any()), "rows that go down, rows that climb"
    assert not bool(moved[0, 0, 1, 1:].any()) and float(stale[0, 0, 32:].max()) > 3, "query block 1 never moves after the first tile"
    _noise_condition(ref_in, None, None, None, 0.0, scale, what=("rising", d), lazy=shift)


def test_the_fully_masked_pairs_have_an_exact_score_contraction():
    """what `packed_inputs_f32(grid_pairs=...)` is for: on the pair it names, q.k summed in fp32 in two halves of d, in reversed order and in fp64
    agree to the bit, so do the scores at -10000; on the other pair they do not"""
    N, heads, d, Tq, Tk = 2, 2, 128, 80, 288
    A, B, dout = F.packed_inputs_f32(N, heads, d, Tq, Tk, grid_pairs=(1,))
    q, k, _, _ = F.packed_views(A, B, dout, N, heads, d, Tq, Tk)
    mask = F.make_mask(N, Tk, "full")
    scale = 1 / math.sqrt(d)
    one, two = F.scores32(q, k, mask, None, scale), F.scores32(q, k, mask, None, scale, halves=True)
    rev = F.scores32(q.flip(-1), k.flip(-1), mask, None, scale)
    wide = F.scores(q, k, mask, None, scale, True)          # q.k in fp64, rounded once
    assert torch.equal(one[1], two[1]) and torch.equal(one[1], rev[1]) and torch.equal(one[1], wide[1])
    assert not torch.equal(one[0], two[0])
    assert float(one[1].max()) < -9990 and float((q[1] / F.GRID).frac().abs().max()) == 0 and float(q[1].abs().max()) < 4


# ---- planted faults ---------------------------------------------------------------------------------------------------------------------------
FACTOR = 5.0


def _big_case():
    N, heads, d, Tq, Tk = 2, 8, 128, 80, 288
    A, B, dout = F.packed_inputs_f32(N, heads, d, Tq, Tk)
    q, k, v, do = F.packed_views(A, B, dout, N, heads, d, Tq, Tk)
    mask = F.make_mask(N, Tk, "tail")
    keep = _keep((N, heads, Tq, Tk), P_DROP, 8)
    scale = 1 / math.sqrt(d)
    exact, emul = F.both(q, k, v, do, mask, None, keep, P_DROP, scale)
    noise = {n: float(F.row_and_block_errors(emul[n], exact[n])[0].max()) for n in F.OUTPUTS}
    return dict(q=q, k=k, v=v, do=do, keep=keep, scale=scale, exact=exact, emul=emul, noise=noise, s=F.scores32(q, k, mask, None, scale))


@pytest.fixture(scope="module")
def big():
    return _big_case()


def _backward(c, keep=None, lse=None, out=None, s=None):
    return F.backward32(c["q"], c["k"], c["v"], c["do"], c["s"] if s is None else s, c["emul"]["lse"] if lse is None else lse,
                        c["emul"]["out"] if out is None else out, c["keep"] if keep is None else keep, P_DROP, c["scale"])


def _caught(name, faulty, c, what, old=None, factor=FACTOR):
    """the per-row statistic of the faulty tensor exceeds MARGIN x noise by `factor`; old: True / False = its whole-tensor relative L2 passes /
    does not pass the 2e-5 of the older tests (None: reported only)"""
    row = float(F.row_and_block_errors(faulty, c["exact"][name])[0].max())
    whole = rel_l2(faulty, c["exact"][name])
    print(f"planted fault {what}: {name} worst row {row:.2e} = {row / c['noise'][name]:.0f} x noise {c['noise'][name]:.2e}, whole-tensor rel l2 {whole:.2e}")
    assert row > factor * F.MARGIN * c["noise"][name], (what, name, row, c["noise"][name])
    if old is not None:
        assert (whole < OLD_BAR) == old, (what, name, whole)
    if old:
        assert rel_l2(c["emul"][name], c["exact"][name]) < whole, "the fault is visible in the whole-tensor figure, just not over its bar"


def test_fault_a_one_key_row_of_dk_misses_one_query_tile(big):
    """dk[pair 1, head 3, key 77] without the contribution of queries 32..63: one wrong row in 4608.  Far over the old criterion too."""
    c = big
    _, dk, _, dS = _backward(c)
    part = (dS[1, 3, 32:64, 77].to(torch.float32) @ c["q"][1, 3, 32:64].to(torch.float32)) * torch.tensor(c["scale"], dtype=torch.float32)
    faulty = dk.clone()
    faulty[1, 3, 77] -= part.double()
    _caught("dk", faulty, c, "a (one query tile missing from one dk row)", old=False)


def _gap_element(c):
    """the keep decision (n, h, i >= 64, j) whose flip moves dq row i by the relative amount closest to 1e-4: over the row bar (about 3e-6) by a wide
    factor, under what the whole-tensor 2e-5 lets one row in 1280 carry (7e-4)"""
    prob = torch.exp(c["s"] - c["emul"]["lse"][..., None])
    dP = c["do"] @ c["v"].transpose(-1, -2)
    d_ds = (prob * dP / (1 - P_DROP)).abs()                                                     # |change of dS| when the decision flips
    rel = d_ds * c["k"].norm(dim=-1)[:, :, None, :] * c["scale"] / c["exact"]["dq"].norm(dim=-1)[..., None]
    rel[:, :, :64] = float("inf")
    rel = torch.where(rel > 0, rel, torch.full_like(rel, float("inf")))
    idx = int((rel.log() - math.log(1e-4)).abs().argmin())
    return tuple(int(x) for x in torch.unravel_index(torch.tensor(idx), rel.shape))


def test_fault_b_one_keep_decision_flipped_in_the_backward_only(big):
    """One keep decision at a query >= 64 (past the second query tile) differs between the forward and a backward body.  In the dQ body it moves one
    row of dq: caught per row and BELOW the old whole-tensor criterion.  In a dK/dV body it moves one row of dk (same) and one of dv, where the change
    is a whole term p * dO / (1 - p) of 80: caught per row; over the old criterion at this size (asserted as such: the gap is in dq and dk)."""
    c = big
    n, h, i, j = _gap_element(c)
    assert i >= 64
    keep = c["keep"].clone()
    keep[n, h, i, j] = 1 - keep[n, h, i, j]
    dq, dk, dv, _ = _backward(c, keep=keep)
    _caught("dq", dq, c, f"b (keep decision {(n, h, i, j)} flipped, dQ body)", old=True)
    _caught("dk", dk, c, f"b (keep decision {(n, h, i, j)} flipped, dK/dV body: dk)", old=True)
    _caught("dv", dv, c, f"b (keep decision {(n, h, i, j)} flipped, dK/dV body: dv)", old=False)


def test_fault_c_one_query_block_exponentiated_against_an_lse_one_step_off(big):
    """queries 32..63 of plane (0, 5), an open pair, read an lse that is off by 2^-10 -- one fp32 step at -10000, where a kernel that forms lse
    around the mask value would lose it: every probability of 32 rows off by a relative 1e-3"""
    c = big
    lse = c["emul"]["lse"].clone()
    lse[0, 5, 32:64] += 2.0 ** -10
    dq, dk, dv, _ = _backward(c, lse=lse)
    _caught("dq", dq, c, "c (lse one step of 2^-10 off for one query block: dq)")
    _caught("dv", dv, c, "c (lse one step of 2^-10 off for one query block: dv)")


def test_fault_d_one_context_row_off_by_ten_times_its_noise(big):
    """one row of the context moved by 10 x the row noise (about 4e-6 of its norm): over the bar of 3 x noise, 75 times under the old one
    (whole-tensor 2.7e-7, most of which is the emulation's own distance from fp64)"""
    c = big
    ref = c["exact"]["out"]
    n, h, i = 1, 6, 70
    g = torch.randn(ref.shape[-1], generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    blk = ref[n, h, 64:80]
    den = max(float(ref[n, h, i].norm()), float((blk ** 2).sum(-1).mean().sqrt()))          # the statistic's denominator (row_and_block_errors)
    faulty = c["emul"]["out"].clone()
    faulty[n, h, i] = ref[n, h, i] + g / g.norm() * 10 * c["noise"]["out"] * den
    _caught("out", faulty, c, "d (one context row off by 10 x noise)", old=True, factor=1.0)


def test_fault_e_one_wrong_grid_step_on_a_fully_masked_pair():
    """Pair 1 fully masked: its scores lie on the fp32 grid of 2^-10 at -10000.  ONE score of the pair one grid step up (a product q.k * scale fused
    with the mask addition does that): one probability off by a relative 1e-3.  Judged as the GPU test judges -- fully masked pair against the emulated
    yardstick, backward from the stored lse -- the row is far over the bar; the same row judged against EXACT fp64 would not even be near it, since
    there the whole pair is 2^-10-grid noise: that is why the yardstick of these pairs is the emulation."""
    N, heads, d, Tq, Tk = 2, 2, 64, 33, 65
    A, B, dout = F.packed_inputs_f32(N, heads, d, Tq, Tk, grid_pairs=(1,))
    ref_in = F.packed_views(A, B, dout, N, heads, d, Tq, Tk)
    q, k, v, do = ref_in
    mask, scale = F.make_mask(N, Tk, "full"), 1 / math.sqrt(d)
    s = F.scores32(q, k, mask, None, scale)
    s[1, 0, 20, 40] += 2.0 ** -10
    out, lse = F.forward32(s, v, None, 0.0, max_shift=F.NOISE_SHIFT)
    dq, dk, dv, _ = F.backward32(q, k, v, do, s, lse, out, None, 0.0, scale)
    res, lres, _, _ = F.verdict(dict(out=out, dq=dq, dk=dk, dv=dv), lse, ref_in, mask, None, None, 0.0, scale, (1,))
    for name, r in res.items():
        print(f"planted fault e (one grid step): {name} row {r['row']:.2e} = {r['row'] / r['noise_row']:.0f} x noise {r['noise_row']:.2e}")
    assert lres["worst"] <= 1.0, "the lse bound alone does not see it"
    for name in ("out", "dv"):
        assert res[name]["row"] > FACTOR * F.MARGIN * res[name]["noise_row"], (name, res[name])
    clean = F.as_dict(F.emulate(q, k, v, do, mask, None, None, 0.0, scale, max_shift=F.NOISE_SHIFT))
    res0, _, _, _ = F.verdict({n: clean[n] for n in F.OUTPUTS}, clean["lse"], ref_in, mask, None, None, 0.0, scale, (1,))
    assert F.within_bar(res0), "without the fault the same evaluation passes"
