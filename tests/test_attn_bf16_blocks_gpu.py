"""GPU: the bf16-resident attention kernels (csrc/attention_bf16.hip) and the bf16 bias-gradient kernel (csrc/attention_dbias.hip) per ROW and per
32-ROW BLOCK against fp64 on the same bf16 inputs and the kernel's own dropout decisions.

The bar is 3 x noise; noise = the rounding-aware emulation of the kernels against exact fp64 (tests/attn_bf16_ref.py), computed here from the
reference alone, never from the kernel.  tests/test_attn_bf16_blocks_cpu.py shows on these very inputs that an independent draw of the kernel's
freedom stays under that bar and that one wrong row, tile or mask word exceeds it by a wide factor while passing the whole-tensor 2e-2 of the older
tests.  Nothing is skipped: fully masked pairs are compared (against the emulated reference, which carries the fp32 score grid at -10000), reference
rows that are identically zero must come back exactly zero, every output and gradient buffer starts as 7.0 and is followed by a guard block of 32
rows of 7.0 that must survive, as must the column blocks next to the addressed one.

With YTVLN_ATTN_ROW_ERRORS=<file> in the environment the measured statistic, the noise and their ratio of every case and output are written to
that file as JSON (profiles/attn_bf16_row_errors.json is one such run)."""
import json
import math
import os

import pytest
import torch

import attn_bf16_ref as R
from test_attn_bias_gpu import make_bias

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GUARD = 32
_RECORDS = []


@pytest.fixture(scope="module", autouse=True)
def _row_error_records():
    yield
    path = os.environ.get("YTVLN_ATTN_ROW_ERRORS")
    if path and _RECORDS:
        with open(path, "w") as f:
            json.dump(dict(margin=R.MARGIN, largest_ratio=max(max(r["ratio_row"], r["ratio_blk"]) for r in _RECORDS), cases=_RECORDS), f, indent=1)


def _rng(dev):
    """a fixed (seed, counter) record as ops.DropoutState hands to the kernels: the decisions do not depend on which tests ran before"""
    return torch.tensor([20250607, 3], dtype=torch.int64, device=dev)


def _guarded(rows, cols, dev):
    return torch.full((rows + GUARD, cols), 7.0, device=dev, dtype=BF)


def _untouched(buf, rows, H, written, what):
    """guard rows and every column block of width H that is not in `written` still hold 7.0"""
    assert bool((buf[rows:] == 7.0).all()), f"{what}: guard rows written"
    for b in range(buf.shape[1] // H):
        if b not in written:
            assert bool((buf[:rows, b * H:(b + 1) * H] == 7.0).all()), f"{what}: column block {b} written"


def _launch(dev, Q, qb, K, kb, V, vb, dout, mask, N, heads, d, Tq, Tk, p=0.0, rng=None, site=0, bias=None):
    """Forward + backward through ops._attn_fwd / ops._attn_bwd.  Q / K / V: 2-D bf16 row tensors (K and V may be one tensor), qb / kb / vb the
    column BLOCKS (of width H) they occupy; gradients go to the same blocks of 7.0-filled buffers of the operands' shapes."""
    from ytvln import ops
    H = heads * d
    scale = 1 / math.sqrt(d)
    out = _guarded(N * Tq, H, dev)
    lse = ops._attn_fwd(Q, qb * H, Q.shape[1], K, kb * H, K.shape[1], V, vb * H, V.shape[1], mask, out, N, heads, Tq, Tk, d, scale, p, rng, site, bias=bias)
    gQ, gK = _guarded(N * Tq, Q.shape[1], dev), _guarded(N * Tk, K.shape[1], dev)
    gV = gK if V is K else _guarded(N * Tk, V.shape[1], dev)
    delta = ops._attn_bwd(Q, qb * H, Q.shape[1], K, kb * H, K.shape[1], V, vb * H, V.shape[1], mask, out, dout, lse, gQ, qb * H, gQ.shape[1],
                          gK, kb * H, gK.shape[1], gV, vb * H, gV.shape[1], N, heads, Tq, Tk, d, scale, p, rng, site, bias=bias)
    torch.cuda.synchronize()
    _untouched(out, N * Tq, H, {0}, "ctx")
    _untouched(gQ, N * Tq, H, {qb}, "dq")
    if V is K:
        _untouched(gK, N * Tk, H, {kb, vb}, "dk | dv")
    else:
        _untouched(gK, N * Tk, H, {kb}, "dk")
        _untouched(gV, N * Tk, H, {vb}, "dv")
    raw = dict(out=out[:N * Tq], dq=gQ[:N * Tq, qb * H:(qb + 1) * H], dk=gK[:N * Tk, kb * H:(kb + 1) * H], dv=gV[:N * Tk, vb * H:(vb + 1) * H])
    got = {n: R.heads_of(t, N, Tq if n in ("out", "dq") else Tk, heads, d) for n, t in raw.items()}
    for n, t in raw.items():
        assert bool(torch.isfinite(t.float()).all()), n
    keep = R.decode_keep(lse._ytvln_keep, N, heads, Tq, Tk) if p > 0 else None
    ref_in = (R.heads_of(Q[:, qb * H:(qb + 1) * H], N, Tq, heads, d), R.heads_of(K[:, kb * H:(kb + 1) * H], N, Tk, heads, d),
              R.heads_of(V[:, vb * H:(vb + 1) * H], N, Tk, heads, d), R.heads_of(dout, N, Tq, heads, d))
    return dict(got=got, raw=raw, lse=lse, keep=keep, delta=delta, ref_in=ref_in, out_buf=out)


def _both(ref_in, mask, bias, keep, p, scale):
    q, k, v, do = ref_in
    return (R.as_dict(R.reference(q, k, v, do, mask, bias, keep, p, scale, False)), R.as_dict(R.reference(q, k, v, do, mask, bias, keep, p, scale, True)))


def _hold(case, run, mask, bias_dense, p, d, full_pairs=()):
    """every output of `run` per row and per block at 3 x noise, its lse at 1e-2 absolute; records the figures, then asserts"""
    scale = 1 / math.sqrt(d)
    exact, emul = _both(run["ref_in"], mask, bias_dense, run["keep"], p, scale)
    noise_from = None
    if len(full_pairs) == exact["out"].shape[0]:
        noise_from = _both(run["ref_in"], None, bias_dense, run["keep"], p, scale)
    res = R.judge(run["got"], exact, emul, full_pairs, noise_from)
    for name, r in res.items():
        rec = dict(case=case, output=name, **r, ratio_row=r["row"] / r["noise_row"], ratio_blk=r["blk"] / r["noise_blk"])
        _RECORDS.append(rec)
        print(f"{case} {name}: row {r['row']:.2e} / noise {r['noise_row']:.2e} = {rec['ratio_row']:.2f}, block {r['blk']:.2e} / {r['noise_blk']:.2e} = "
              f"{rec['ratio_blk']:.2f}, all-zero reference blocks {r['zero_blocks']}, exact zeros {r['zeros_exact']}")
    lse_err = float((run["lse"].double() - exact["lse"]).abs().max())
    for name, r in res.items():
        assert r["zeros_exact"], (case, name, "a reference row that is identically zero came back non-zero")
        assert r["row"] <= R.MARGIN * r["noise_row"], (case, name, "row", r)
        assert r["blk"] <= R.MARGIN * r["noise_blk"], (case, name, "block", r)
    assert lse_err < 1e-2, (case, "lse", lse_err)
    return exact, emul


# ---- A: granule edges ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", R.MASKS)
@pytest.mark.parametrize("N,heads,d,Tq,Tk", R.SHAPES_EDGES)
def test_granule_edges(dev, lib, N, heads, d, Tq, Tk, pattern):
    """One query, 31 / 32 / 33 / 65 queries or keys, ragged last tiles on either side, many key tiles; a padded tail, masked LEADING keys (the
    running maximum starts near -10000 and jumps by 10^4 in a later tile or inside the first one), and a fully masked pair."""
    A, B, dout = (t.to(dev) for t in R.packed_inputs(N, heads, d, Tq, Tk))
    mask = R.make_mask(N, Tk, pattern).to(dev)
    run = _launch(dev, A, R.Q_OFF, B, R.K_OFF, B, R.V_OFF, dout, mask, N, heads, d, Tq, Tk)
    exact, _ = _hold(f"edges N{N} h{heads} d{d} Tq{Tq} Tk{Tk} {pattern}", run, mask, None, 0.0, d, (N - 1,) if pattern == "full" else ())
    if pattern != "full":          # keys under the mask: their dk / dv rows are identically zero in the reference, hence asserted exactly zero above
        masked = (mask != 0)[:, None, :].expand(N, heads, Tk)
        assert bool((exact["dk"].abs().amax(-1)[masked] == 0).all()) and bool(masked.any())


# ---- B: rising maxima ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128])
def test_rising_maxima(dev, lib, d):
    """Scores a_i c_j with c_j stepping up at every key tile (attn_bf16_ref.rising_inputs): inside one 32-query block the wave moves its softmax
    reference at some tiles and not at others, rows in it are stale by up to 12, others have their maximum in the first tile.  Separate q / k / v."""
    N, heads, Tq, Tk = 2, 2, 64, 160
    q, k, v, dout = (t.to(dev) for t in R.rising_inputs(d))
    run = _launch(dev, q, 0, k, 0, v, 0, dout, None, N, heads, d, Tq, Tk)
    s = R.scores(run["ref_in"][0], run["ref_in"][1], None, None, 1 / math.sqrt(d), True)
    _, stale, moved = R.lazy_shift(s)
    b0 = moved[0, 0, 0]
    assert bool(b0[1:].any()) and not bool(b0[1:].all()) and float(stale[0, 0, :32].max()) > 3, "the construction takes both branches in one block"
    _hold(f"rising d{d}", run, None, None, 0.0, d)


# ---- C: dropout at ragged, multi-tile shapes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("N,heads,d,Tq,Tk", R.SHAPES_DROP)
def test_dropout_ragged_multi_tile(dev, lib, N, heads, d, Tq, Tk, p):
    """The stored keep masks [pair * head][query block][key tile][16] with a ragged last key tile, a ragged last query block and up to 9 tiles:
    decoded from the buffer == recovered from the bf16 kernel's output == recovered from the fp32 kernel's output (same rng record and site).
    Keep rate within 0.02 of 1 - p: a condition on the inputs -- sigma = sqrt(p (1 - p) / n), so 0.02 is > 5 sigma from n = 15625 decisions at
    p = 0.5 and n = 5625 at p = 0.1.  The shapes hold 14948 (4.9 sigma at p = 0.5, 8.2 at 0.1), 45600 and 38016; the whole buffer, whose bits
    past the ragged ends are draws of the same hash, holds 32768 at the first shape and is held to the same 0.02 (7.2 sigma).
    Then out / dq / dk / dv per row with that mask."""
    from ytvln import ops
    rng, site = _rng(dev), 5
    A, B, dout = (t.to(dev) for t in R.packed_inputs(N, heads, d, Tq, Tk))
    mask = R.make_mask(N, Tk, "tail").to(dev)
    run = _launch(dev, A, R.Q_OFF, B, R.K_OFF, B, R.V_OFF, dout, mask, N, heads, d, Tq, Tk, p=p, rng=rng, site=site)
    keep = run["keep"]
    from_bf16 = R.recover_keep(ops._attn_fwd, dev, BF, N, heads, d, Tq, Tk, p, rng, site)
    from_fp32 = R.recover_keep(ops._attn_fwd, dev, torch.float32, N, heads, d, Tq, Tk, p, rng, site)
    assert torch.equal(keep, from_bf16), "the stored masks are not the decisions the bf16 forward applied"
    assert torch.equal(from_bf16, from_fp32), "bf16 and fp32 kernels must draw the same mask"
    assert abs(float(keep.mean()) - (1 - p)) < 0.02, float(keep.mean())
    nb, nt = -(-Tq // 32), -(-Tk // 32)
    whole = R.decode_keep(run["lse"]._ytvln_keep, N, heads, nb * 32, nt * 32)
    assert abs(float(whole.mean()) - (1 - p)) < 0.02, float(whole.mean())
    _hold(f"dropout p{p} N{N} h{heads} d{d} Tq{Tq} Tk{Tk}", run, mask, None, p, d)


# ---- D: pair launch -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [None, 1])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("d", [64, 128])
def test_pair_launch_forward_and_backward(dev, lib, d, p, side):
    """CoAttentionFn (both directions of BertBiAttention in one launch per kernel), R = 70 regions, T = 45 tokens: contexts, log-sum-exps AND the
    four gradients equal the two single launches bit for bit, with dropout off and on and (side = 1) a co-attention bias on the first direction
    only; the single launches hold the per-row bar."""
    from ytvln import ops
    N, Rr, T, heads = 2, 70, 45, 2
    Hb = heads * d
    q1, kv1, q2, kv2, m1, m2, g1, g2 = (t.to(dev) for t in R.pair_inputs(N, Rr, T, heads, d))
    rng = _rng(dev) if p > 0 else None
    bias1 = dense1 = None
    if side == 1:
        co, dense = make_bias(dev, "n1", N, heads, Rr, T, seed=21)
        bias1, dense1 = co.transpose(2, 3), dense.transpose(2, 3)
    leaves = [t.clone().requires_grad_() for t in (q1, kv1, q2, kv2)]
    c1, c2, l1, l2 = ops.CoAttentionFn.apply(*leaves, m1, m2, N, Rr, T, heads, p, p, rng, 7, 8, *(() if side is None else (bias1, None)))
    torch.autograd.backward([c1, c2], [g1, g2])
    gq1, gkv1, gq2, gkv2 = (t.grad for t in leaves)
    a = _launch(dev, q2, 0, kv1, 0, kv1, 1, g1, m1, N, heads, d, T, Rr, p=p, rng=rng, site=7, bias=bias1)          # text queries over regions
    b = _launch(dev, q1, 0, kv2, 0, kv2, 1, g2, m2, N, heads, d, Rr, T, p=p, rng=rng, site=8)                      # region queries over tokens
    for x, y, what in ((c1.detach(), a["raw"]["out"], "ctx1"), (c2.detach(), b["raw"]["out"], "ctx2"), (l1, a["lse"], "lse1"), (l2, b["lse"], "lse2"),
                       (gq2, a["raw"]["dq"], "dq2"), (gkv1[:, :Hb], a["raw"]["dk"], "dk1"), (gkv1[:, Hb:], a["raw"]["dv"], "dv1"),
                       (gq1, b["raw"]["dq"], "dq1"), (gkv2[:, :Hb], b["raw"]["dk"], "dk2"), (gkv2[:, Hb:], b["raw"]["dv"], "dv2")):
        assert torch.equal(x, y), (what, float((x.float() - y.float()).abs().max()))
    _hold(f"pair d{d} p{p} bias {side} text-over-regions", a, m1, dense1, p, d)
    _hold(f"pair d{d} p{p} bias {side} regions-over-text", b, m2, None, p, d)


# ---- E: bias forms ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["nh", "n1T"])
@pytest.mark.parametrize("N,heads,d,Tq,Tk", R.SHAPES_BIAS)
def test_bias_forms(dev, lib, N, heads, d, Tq, Tk, form):
    """A per-score bias ([N, heads, Tq, Tk] and the transposed view of [N, 1, Tk, Tq]) with its -10000 and -inf entries left in, plus one key whose
    whole column is -inf in one plane: its dk and dv rows depend on nothing but zeros of dS and P and must be exactly zero."""
    A, B, dout = (t.to(dev) for t in R.packed_inputs(N, heads, d, Tq, Tk))
    mask = R.make_mask(N, Tk, "tail").to(dev)
    bias, _ = make_bias(dev, form, N, heads, Tq, Tk)
    dense = R.with_inf_column(bias).double().expand(N, heads, Tq, Tk)
    run = _launch(dev, A, R.Q_OFF, B, R.K_OFF, B, R.V_OFF, dout, mask, N, heads, d, Tq, Tk, bias=bias)
    exact, _ = _hold(f"bias {form} N{N} h{heads} d{d} Tq{Tq} Tk{Tk}", run, mask, dense, 0.0, d)
    assert bool(torch.isinf(dense).any()) and float(exact["dS"][torch.isinf(dense)].abs().max()) == 0
    hs = range(heads) if form == "n1T" else [heads - 1]
    for h in hs:
        assert float(exact["dk"][0, h, R.INF_KEY].abs().max()) == 0 and float(exact["dv"][0, h, R.INF_KEY].abs().max()) == 0
        assert float(run["got"]["dk"][0, h, R.INF_KEY].abs().max()) == 0 and float(run["got"]["dv"][0, h, R.INF_KEY].abs().max()) == 0


# ---- F: layout independence ---------------------------------------------------------------------------------------------------------------------
def test_packed_and_separate_operands_give_the_same_bits(dev, lib):
    N, heads, d, Tq, Tk = 2, 2, 64, 33, 65
    H = heads * d
    A, B, dout = (t.to(dev) for t in R.packed_inputs(N, heads, d, Tq, Tk))
    mask = R.make_mask(N, Tk, "tail").to(dev)
    packed = _launch(dev, A, R.Q_OFF, B, R.K_OFF, B, R.V_OFF, dout, mask, N, heads, d, Tq, Tk)
    q, k, v = (t[:, b * H:(b + 1) * H].contiguous() for t, b in ((A, R.Q_OFF), (B, R.K_OFF), (B, R.V_OFF)))
    separate = _launch(dev, q, 0, k, 0, v, 0, dout, mask, N, heads, d, Tq, Tk)
    assert torch.equal(packed["lse"], separate["lse"])
    for name in R.OUTPUTS:
        assert torch.equal(packed["raw"][name], separate["raw"][name]), name


# ---- G: bias gradient ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("N,heads,d,Tq,Tk", R.SHAPES_DBIAS)
def test_bias_gradient_per_block(dev, lib, N, heads, d, Tq, Tk, p):
    """ytvln_attn_dbias_bf16, gradient layout [N, heads, Tq, Tk]: dBias per (pair, head, 32-query block) against the reference dS.  The kernel
    writes fp32, so the noise is the emulated dS BEFORE its bf16 rounding against the exact one (what is left: the bf16 context inside delta, the
    fp32 log-sum-exp and score).  Entries under a -inf bias are exactly zero.  (p = 0.1: the kernel's own reading of the stored keep masks.)"""
    from ytvln import ops
    H = heads * d
    scale = 1 / math.sqrt(d)
    rng = _rng(dev) if p > 0 else None
    A, B, dout = (t.to(dev) for t in R.packed_inputs(N, heads, d, Tq, Tk, seed=R.DBIAS_SEED))
    mask = R.make_mask(N, Tk, "tail").to(dev)
    bias, dense = make_bias(dev, "nh", N, heads, Tq, Tk)
    run = _launch(dev, A, R.Q_OFF, B, R.K_OFF, B, R.V_OFF, dout, mask, N, heads, d, Tq, Tk, p=p, rng=rng, site=9, bias=bias)
    pr = ops._attn_problem(A, R.Q_OFF * H, 3 * H, B, R.K_OFF * H, 3 * H, B, R.V_OFF * H, 3 * H, mask, Tq, Tk, p, 9, ctx_in=run["out_buf"], dctx=dout,
                           lse_in=run["lse"], delta=run["delta"], keep=getattr(run["lse"], "_ytvln_keep", None))
    g = ops._attn_dbias(pr, bias, ((N, heads, Tq, Tk), torch.float32), True, N, heads, Tq, Tk, d, scale, rng, dev)
    torch.cuda.synchronize()
    assert g.dtype == torch.float32 and bool(torch.isfinite(g).all())
    exact, emul = _both(run["ref_in"], mask, dense, run["keep"], p, scale)
    row, blk, zero = R.row_and_block_errors(g, exact["dS"])
    nrow, nblk, _ = R.row_and_block_errors(emul["dS"], exact["dS"])
    rec = dict(case=f"dbias p{p} N{N} h{heads} d{d} Tq{Tq} Tk{Tk}", output="dbias", row=float(row.max()), blk=float(blk.max()), noise_row=float(nrow.max()),
               noise_blk=float(nblk.max()), zero_blocks=int(zero.sum()), zeros_exact=True, ratio_row=float(row.max() / nrow.max()),
               ratio_blk=float(blk.max() / nblk.max()))
    _RECORDS.append(rec)
    print(rec)
    assert int(zero.sum()) == 0
    assert float(g[torch.isinf(dense)].abs().max()) == 0.0, "entries under a -inf bias get exactly 0"
    assert rec["blk"] <= R.MARGIN * rec["noise_blk"], rec
