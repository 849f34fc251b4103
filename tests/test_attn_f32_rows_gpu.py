"""GPU: the fp32 attention kernels (csrc/attention.hip) per ROW and per 32-ROW BLOCK against fp64 on the same inputs and the kernel's own dropout
decisions, under every kernel form the library's run-time options select.

The bar is MARGIN = 3 x noise; noise = the fp32 emulation of the kernels against exact fp64 (tests/attn_f32_ref.py), computed here from the
reference alone, never from the kernel.  tests/test_attn_f32_rows_cpu.py shows on these very inputs that five independent fp32 orders of the same
mathematics stay under that bar and that one wrong row, query tile, keep decision, lse step or score grid step exceeds it, where the whole-tensor 2e-5
of test_attention_fwd_bwd / test_attention_dropout lets the smaller of them pass.  Nothing is skipped: fully masked pairs are compared (against the
emulated reference, which carries the fp32 score grid at -10000; their backward against the emulated backward from the stored lse), reference rows
that are identically zero must come back exactly zero, every output and gradient buffer starts as 7.0 and is followed by a guard block of 32 rows
of 7.0 that must survive, as must the column blocks next to the addressed one.  lse is held per row to 3 x its noise plus one fp32 step, and
ops.attn_probs per row by the same rule on the edge cases.

With YTVLN_ATTN_F32_ROW_ERRORS=<file> in the environment the measured statistic, the noise and their ratio of every case, form and output are
written to that file as JSON (profiles/attn_f32_row_errors.json is one such run)."""
import json
import math
import os

import pytest
import torch

import attn_f32_ref as F
from test_attn_bias_gpu import make_bias

pytestmark = pytest.mark.gpu
F32 = torch.float32
GUARD = 32
_RECORDS = []
_BASE = {}          # case -> attn_f32_ref.reference_base: computed once, shared by the forms, never written to

FORMS = {
    "default": {},                                                    # the planner's choice
    "w1_any": {"ATTN_W1_DKV_ANY": 1},                                 # one-wave forward / dK/dV + stored dS at small shapes
    "w1_recompute": {"ATTN_W1": 7, "ATTN_W1_DKV_ANY": 1},             # one-wave kernels, recomputing dQ
    "two_wave": {"ATTN_W1": 0},                                       # multi-wave forward / dQ with d-split, wave-pair dK/dV
    "two_wave_nosplit": {"ATTN_W1": 0, "ATTN_DSPLIT": 0},             # the same without the d-split
}
ALL_FORMS = list(FORMS)
SOME_FORMS = ["default", "w1_any", "two_wave"]


class _Form:
    def __init__(self, name):
        from ytvln import _lib
        self.name, self._lib = name, _lib
        self.prev = {}
        try:
            for k, v in FORMS[name].items():
                self.prev[k] = _lib.set_option(k, v)
                assert _lib.set_option(k, v) == v, (k, "the option did not take")
        except BaseException:
            self.restore()          # (no option of a half-set form leaks into later tests)
            raise

    def restore(self):
        for k, v in self.prev.items():
            self._lib.set_option(k, v)


@pytest.fixture
def form(request, lib):
    f = _Form(request.param)
    yield f.name
    f.restore()


@pytest.fixture(scope="module", autouse=True)
def _row_error_records():
    yield
    _BASE.clear()
    path = os.environ.get("YTVLN_ATTN_F32_ROW_ERRORS")
    if path and _RECORDS:
        _write_records(path, _RECORDS)


def _write_records(path, records):
    """the bf16 file's layout (margin, largest_ratio, cases: one record per case, form and output), one record per line, figures to four digits;
    forms whose figures for a case and output are identical to the digit (they ran the same kernel body) share a record, `form` naming them all"""
    def short(r):
        return {k: float(f"{v:.4g}") if isinstance(v, float) else v for k, v in r.items()}
    merged = {}
    for r in map(short, records):
        key = json.dumps({k: v for k, v in r.items() if k != "form"})
        if key in merged:
            merged[key]["form"] += "+" + r["form"]
        else:
            merged[key] = r
    largest = max(max(r["ratio_row"], r["ratio_blk"]) for r in records)
    with open(path, "w") as f:
        f.write('{"margin": %s, "largest_ratio": %.4g, "records": %d, "cases": [\n' % (json.dumps(F.MARGIN), largest, len(records)))
        f.write(",\n".join(json.dumps(r) for r in merged.values()))
        f.write("\n]}\n")


def _rng(dev):
    """a fixed (seed, counter) record as ops.DropoutState hands to the kernels: the decisions do not depend on which tests ran before"""
    return torch.tensor([20250607, 3], dtype=torch.int64, device=dev)


def _guarded(rows, cols, dev):
    return torch.full((rows + GUARD, cols), 7.0, device=dev, dtype=F32)


def _untouched(buf, rows, H, written, what):
    """guard rows and every column block of width H that is not in `written` still hold 7.0"""
    assert bool((buf[rows:] == 7.0).all()), f"{what}: guard rows written"
    for b in range(buf.shape[1] // H):
        if b not in written:
            assert bool((buf[:rows, b * H:(b + 1) * H] == 7.0).all()), f"{what}: column block {b} written"


def _collect(raw, ins, N, heads, d, Tq, Tk):
    """raw: name -> 2-D row tensors of one problem; ins: (q, k, v, dout) 2-D slices -> the `run` dict the checks take"""
    for n, t in raw.items():
        assert bool(torch.isfinite(t).all()), n
    got = {n: F.heads_of(t, N, Tq if n in ("out", "dq") else Tk, heads, d) for n, t in raw.items()}
    ref_in = tuple(F.heads_of(x, N, T, heads, d) for x, T in zip(ins, (Tq, Tk, Tk, Tq)))
    return dict(got=got, raw=raw, ref_in=ref_in)


def _launch(dev, Q, qb, K, kb, V, vb, dout, mask, N, heads, d, Tq, Tk, p=0.0, rng=None, site=0, bias=None):
    """Forward + backward through ops._attn_fwd / ops._attn_bwd.  Q / K / V: 2-D fp32 row tensors (K and V may be one tensor), qb / kb / vb the
    column BLOCKS (of width H) they occupy; gradients go to the same blocks of 7.0-filled buffers of the operands' shapes."""
    from ytvln import ops
    H = heads * d
    scale = 1 / math.sqrt(d)
    out = _guarded(N * Tq, H, dev)
    lse = ops._attn_fwd(Q, qb * H, Q.shape[1], K, kb * H, K.shape[1], V, vb * H, V.shape[1], mask, out, N, heads, Tq, Tk, d, scale, p, rng, site, bias=bias)
    gQ, gK = _guarded(N * Tq, Q.shape[1], dev), _guarded(N * Tk, K.shape[1], dev)
    gV = gK if V is K else _guarded(N * Tk, V.shape[1], dev)
    ops._attn_bwd(Q, qb * H, Q.shape[1], K, kb * H, K.shape[1], V, vb * H, V.shape[1], mask, out, dout, lse, gQ, qb * H, gQ.shape[1],
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
    run = _collect(raw, (Q[:, qb * H:(qb + 1) * H], K[:, kb * H:(kb + 1) * H], V[:, vb * H:(vb + 1) * H], dout), N, heads, d, Tq, Tk)
    assert lse.dtype == F32 and bool(torch.isfinite(lse).all())
    run["lse"] = lse
    return run


def _hold(case, form, run, mask, bias_dense, keep, p, d, full_pairs=(), share=True):
    """every output of `run` per row and per block at MARGIN x noise, its lse per row; records the figures, then asserts"""
    scale = 1 / math.sqrt(d)
    base = _BASE.get(case) if share else None
    if base is None:
        base = F.reference_base(run["ref_in"], mask, bias_dense, keep, p, scale, full_pairs)
        if share:
            _BASE[case] = base
    res, lres, exact, emul = F.verdict(run["got"], run["lse"], run["ref_in"], mask, bias_dense, keep, p, scale, full_pairs, base=base)
    for name, r in res.items():
        rec = dict(case=case, form=form, output=name, **r, ratio_row=r["row"] / r["noise_row"], ratio_blk=r["blk"] / r["noise_blk"])
        _RECORDS.append(rec)
        print(f"{case} [{form}] {name}: row {r['row']:.2e} / noise {r['noise_row']:.2e} = {rec['ratio_row']:.2f}, block {r['blk']:.2e} / {r['noise_blk']:.2e} = "
              f"{rec['ratio_blk']:.2f}, all-zero reference blocks {r['zero_blocks']}, exact zeros {r['zeros_exact']}")
    print(f"{case} [{form}] lse: err {lres['err']:.2e}, noise {lres['noise']:.2e}, worst err / bound {lres['worst']:.2f}")
    for name, r in res.items():
        assert r["zeros_exact"], (case, form, name, "a reference row that is identically zero came back non-zero")
        assert r["row"] <= F.MARGIN * r["noise_row"], (case, form, name, "row", r)
        assert r["blk"] <= F.MARGIN * r["noise_blk"], (case, form, name, "block", r)
    assert lres["worst"] <= 1.0, (case, form, "lse", lres)
    return exact, emul


def _hold_probs(case, form, dev, run, Q, qb, K, kb, mask, N, heads, d, Tq, Tk, exact, emul, full_pairs):
    """ops.attn_probs (exp(s - lse) from the forward's lse) per query row and 32-row block, by the rule of the outputs: open pairs against
    exact fp64, fully masked pairs against the emulation from the stored lse, at MARGIN x (emulated against exact over the open pairs)"""
    from ytvln import ops
    H = heads * d
    scale = 1 / math.sqrt(d)
    probs = ops.attn_probs(Q, qb * H, Q.shape[1], K, kb * H, K.shape[1], mask, run["lse"], N, heads, Tq, Tk, d, scale)
    torch.cuda.synchronize()
    _judge_probs(case, form, probs, run, mask, N, heads, Tq, Tk, scale, exact, emul, full_pairs)


def _judge_probs(case, form, probs, run, mask, N, heads, Tq, Tk, scale, exact, emul, full_pairs):
    assert probs.dtype == F32 and tuple(probs.shape) == (N, heads, Tq, Tk) and bool(torch.isfinite(probs).all())
    q, k = run["ref_in"][:2]
    s_ex, s_em = F.scores(q, k, mask, None, scale, False), F.scores32(q, k, mask, None, scale)
    ex = dict(probs=F.probs_of(s_ex, exact["lse"], False))
    em = dict(probs=F.probs_of(s_em, emul["lse"], True))
    for n in full_pairs:
        em["probs"][n] = F.probs_of(s_em[n], run["lse"][n].double(), True)
    noise_from = None
    if len(full_pairs) == N:
        nf_ex, nf_em, _ = F.reference_base(run["ref_in"], None, None, None, 0.0, scale)
        noise_from = (dict(probs=F.probs_of(F.scores(q, k, None, None, scale, False), nf_ex["lse"], False)),
                      dict(probs=F.probs_of(F.scores32(q, k, None, None, scale), nf_em["lse"], True)))
    r = F.judge(dict(probs=probs.double()), ex, em, full_pairs, noise_from)["probs"]
    rec = dict(case=case, form=form, output="probs", **r, ratio_row=r["row"] / r["noise_row"], ratio_blk=r["blk"] / r["noise_blk"])
    _RECORDS.append(rec)
    print(f"{case} [{form}] probs: row {r['row']:.2e} / noise {r['noise_row']:.2e} = {rec['ratio_row']:.2f}, block {rec['ratio_blk']:.2f}")
    assert r["row"] <= F.MARGIN * r["noise_row"] and r["blk"] <= F.MARGIN * r["noise_blk"], (case, form, "probs", r)
    assert float((probs.sum(-1) - 1).abs().max()) < 2e-3, "rows of probabilities sum to 1 (to the lse step at -10000)"


# ---- the forms are what they say ------------------------------------------------------------------------------------------------------------------
def test_every_form_runs_kernels_of_its_own(dev, lib):
    """(2, 2, 128, 65, 33): three query tiles, so the two-wave forward's second workgroup holds ONE tile and sums the head dimension in two halves
    (the d-split) -- other bits than the one-wave forward of `default`, and than `two_wave_nosplit`.  The stored-dS backward is what `w1_any` adds to
    `default` at this size and what `w1_recompute` takes away again: the planner's workspace size says so.  `w1_recompute` against `default`: both
    plan no workspace here and their kernels sum in the same order, so their bits are equal by design -- the only evidence for that form is that
    its options took (`_Form`) and that they move the planner away from `w1_any`."""
    N, heads, d, Tq, Tk = 2, 2, 128, 65, 33
    A, B, dout = (t.to(dev) for t in F.packed_inputs_f32(N, heads, d, Tq, Tk))
    mask = F.make_mask(N, Tk, "tail").to(dev)
    runs, ws = {}, {}
    for name in ALL_FORMS:
        f = _Form(name)
        try:
            ws[name] = int(lib.ytvln_attn_bwd_workspace_elems(N, heads, d, Tq, Tk, 0, 0))
            runs[name] = _launch(dev, A, F.Q_OFF, B, F.K_OFF, B, F.V_OFF, dout, mask, N, heads, d, Tq, Tk)
        finally:
            f.restore()
    same = {name: {n: torch.equal(runs[name]["raw"][n], runs["default"]["raw"][n]) for n in F.OUTPUTS} for name in ALL_FORMS}
    print("workspace floats", ws, "bits equal to default", same)
    assert ws["default"] == 0 and ws["w1_any"] == N * heads * 3 * 2 * 1024 and ws["w1_recompute"] == 0 and ws["two_wave"] == 0
    assert not same["two_wave"]["out"], "ATTN_W1 = 0: the d-split forward sums in another order than the one-wave forward"
    split, whole = runs["two_wave"]["got"]["out"], runs["two_wave_nosplit"]["got"]["out"]
    assert not torch.equal(split[:, :, 64:], whole[:, :, 64:]), "ATTN_DSPLIT = 0 takes the d-split away"
    assert torch.equal(split[:, :, :64], whole[:, :, :64]), "... and changes nothing in whole workgroups"


def test_d_split_runs_past_512_keys(dev, lib):
    """(1, 2, 128, 65, 576): past 512 keys every form, `default` included, takes the multi-wave forward, whose second workgroup holds ONE query
    tile (query 64) and runs the d-split with its 4 KB score exchange BEHIND a mask row of 576 floats.  That it ran: `two_wave` (and `default`)
    differ in bits from `two_wave_nosplit` in that workgroup's row and nowhere else.  (33 or 40 queries do not reach it: two tiles, one workgroup.)"""
    N, heads, d, Tq, Tk = 1, 2, 128, 65, 576
    A, B, dout = (t.to(dev) for t in F.packed_inputs_f32(N, heads, d, Tq, Tk))
    mask = F.make_mask(N, Tk, "tail").to(dev)
    out = {}
    for name in ("default", "two_wave", "two_wave_nosplit"):
        f = _Form(name)
        try:
            out[name] = _launch(dev, A, F.Q_OFF, B, F.K_OFF, B, F.V_OFF, dout, mask, N, heads, d, Tq, Tk)["got"]["out"]
        finally:
            f.restore()
    for name in ("default", "two_wave"):
        assert not torch.equal(out[name][:, :, 64:], out["two_wave_nosplit"][:, :, 64:]), (name, "the d-split did not run")
        assert torch.equal(out[name][:, :, :64], out["two_wave_nosplit"][:, :, :64]), name


# ---- A: granule edges ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ALL_FORMS, indirect=True)
@pytest.mark.parametrize("pattern", F.MASKS)
@pytest.mark.parametrize("N,heads,d,Tq,Tk", F.SHAPES_EDGES_F32)
def test_granule_edges(dev, lib, form, N, heads, d, Tq, Tk, pattern):
    """One query, 31 / 32 / 33 / 65 queries or keys, ragged last tiles on either side, many key tiles, padded heads (DP = 32 / 64 / 128), more than
    512 keys; a padded tail, masked LEADING keys (the running maximum starts near -10000 and jumps by 10^4), and a fully masked pair.  A shape a
    form's kernels do not exist for falls through to the other bodies and is held all the same."""
    full = (N - 1,) if pattern == "full" else ()
    A, B, dout = (t.to(dev) for t in F.packed_inputs_f32(N, heads, d, Tq, Tk, seed=F.edge_seed((N, heads, d, Tq, Tk)), grid_pairs=full))
    mask = F.make_mask(N, Tk, pattern).to(dev)
    run = _launch(dev, A, F.Q_OFF, B, F.K_OFF, B, F.V_OFF, dout, mask, N, heads, d, Tq, Tk)
    case = f"edges N{N} h{heads} d{d} Tq{Tq} Tk{Tk} {pattern}"
    exact, emul = _hold(case, form, run, mask, None, None, 0.0, d, full)
    if pattern != "full":          # keys under the mask: their dk / dv rows are identically zero in the reference, hence asserted exactly zero above
        masked = (mask != 0)[:, None, :].expand(N, heads, Tk)
        assert bool((exact["dk"].abs().amax(-1)[masked] == 0).all()) and bool(masked.any())
    _hold_probs(case, form, dev, run, A, F.Q_OFF, B, F.K_OFF, mask, N, heads, d, Tq, Tk, exact, emul, full)


# ---- B: rising maxima ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ALL_FORMS, indirect=True)
@pytest.mark.parametrize("d", [64, 128])
def test_rising_maxima(dev, lib, form, d):
    """Scores a_i c_j with c_j stepping up at every key tile (attn_f32_ref.rising_inputs_f32): inside one 32-query block the wave moves its softmax
    reference at some tiles and not at others, rows in it are stale by up to 12, others have their maximum in the first tile -- the one numerical
    freedom of the four forward bodies, exercised.  Separate q / k / v."""
    N, heads, Tq, Tk = 2, 2, 64, 160
    q, k, v, dout = (t.to(dev) for t in F.rising_inputs_f32(d))
    run = _launch(dev, q, 0, k, 0, v, 0, dout, None, N, heads, d, Tq, Tk)
    s = F.scores32(run["ref_in"][0], run["ref_in"][1], None, None, 1 / math.sqrt(d))
    _, stale, moved = F.lazy_shift(s)
    b0 = moved[0, 0, 0]
    assert bool(b0[1:].any()) and not bool(b0[1:].all()) and float(stale[0, 0, :32].max()) > 3, "the construction takes both branches in one block"
    _hold(f"rising d{d}", form, run, None, None, None, 0.0, d)


# ---- C: dropout at ragged, multi-tile shapes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", SOME_FORMS, indirect=True)
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("N,heads,d,Tq,Tk", F.SHAPES_DROP_F32)
def test_dropout_ragged_multi_tile(dev, lib, form, N, heads, d, Tq, Tk, p):
    """The backward bodies apply the decisions the forward drew, element by element: the forward hashes (key, score row), the dK/dV bodies
    (key, first row of the problem + query tile + krow) -- past the second query tile, in ragged tiles on either side, at a padded head size and past
    512 keys.  The keep decisions are recovered from the forward's OUTPUT (`recover_keep`: same form, same rng record and site); then out / dq / dk /
    dv per row with that mask.
    Keep rate within 0.02 of 1 - p: a condition on the inputs.  sigma = sqrt(p (1 - p) / n); the shapes hold n = 14948, 45600, 38016, 12870, 46080
    and 14800 decisions, so 0.02 is at least 4.5 sigma at p = 0.5 (sigma <= 4.4e-3 at n = 12870) and at least 7.5 sigma at p = 0.1
    (sigma <= 2.7e-3): no seed had to be redrawn."""
    from ytvln import ops
    rng, site = _rng(dev), 5
    A, B, dout = (t.to(dev) for t in F.packed_inputs_f32(N, heads, d, Tq, Tk))
    mask = F.make_mask(N, Tk, "tail").to(dev)
    run = _launch(dev, A, F.Q_OFF, B, F.K_OFF, B, F.V_OFF, dout, mask, N, heads, d, Tq, Tk, p=p, rng=rng, site=site)
    keep = F.recover_keep(ops._attn_fwd, dev, F32, N, heads, d, Tq, Tk, p, rng, site)
    assert abs(float(keep.mean()) - (1 - p)) < 0.02, float(keep.mean())
    _hold(f"dropout p{p} N{N} h{heads} d{d} Tq{Tq} Tk{Tk}", form, run, mask, None, keep, p, d, share=False)


# ---- D: pair launch -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", SOME_FORMS, indirect=True)
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("Rr,T", F.PAIR_RT)
def test_pair_launch_forward_and_backward(dev, lib, form, Rr, T, d, p):
    """Both directions of BertBiAttention in one launch per kernel, R = 72 regions and T = 20 tokens and the reverse, so that the launches' ordering
    of the two problems (long keys first for the forward and dQ, long queries first for dK/dV) swaps them either way.  Once through the pair entry
    points into guarded buffers, once through ops.CoAttentionFn: the same bits; each direction per row against fp64 -- with dropout against the
    decisions a SINGLE forward launch of that direction draws, which the second problem of a pair must reproduce from its own row ids."""
    from ytvln import ops
    N, heads = 2, 2
    Hb = heads * d
    scale = 1 / math.sqrt(d)
    q1, kv1, q2, kv2, m1, m2, g1, g2 = (t.to(dev) for t in F.pair_inputs_f32(N, Rr, T, heads, d))
    rng = _rng(dev) if p > 0 else None
    ctx1, ctx2 = _guarded(N * T, Hb, dev), _guarded(N * Rr, Hb, dev)
    lse1, lse2 = torch.empty(N, heads, T, device=dev), torch.empty(N, heads, Rr, device=dev)
    ops._attn_launch(False, False, ops._attn_problem(q2, 0, Hb, kv1, 0, 2 * Hb, kv1, Hb, 2 * Hb, m1, T, Rr, p, 7, ctx=ctx1, lse=lse1),
                     ops._attn_problem(q1, 0, Hb, kv2, 0, 2 * Hb, kv2, Hb, 2 * Hb, m2, Rr, T, p, 8, ctx=ctx2, lse=lse2), N, heads, d, scale, rng)
    gq2, gkv1, gq1, gkv2 = _guarded(N * T, Hb, dev), _guarded(N * Rr, 2 * Hb, dev), _guarded(N * Rr, Hb, dev), _guarded(N * T, 2 * Hb, dev)
    dl1, dl2 = torch.empty_like(lse1), torch.empty_like(lse2)
    ops._attn_launch(True, False,
                     ops._attn_problem(q2, 0, Hb, kv1, 0, 2 * Hb, kv1, Hb, 2 * Hb, m1, T, Rr, p, 7, ctx_in=ctx1, dctx=g1, lse_in=lse1, delta=dl1,
                                       dq=gq2, lddq=Hb, dk=gkv1, lddk=2 * Hb, dv=gkv1, dv_off=Hb, lddv=2 * Hb),
                     ops._attn_problem(q1, 0, Hb, kv2, 0, 2 * Hb, kv2, Hb, 2 * Hb, m2, Rr, T, p, 8, ctx_in=ctx2, dctx=g2, lse_in=lse2, delta=dl2,
                                       dq=gq1, lddq=Hb, dk=gkv2, lddk=2 * Hb, dv=gkv2, dv_off=Hb, lddv=2 * Hb), N, heads, d, scale, rng)
    torch.cuda.synchronize()
    for buf, rows, what in ((ctx1, N * T, "ctx1"), (ctx2, N * Rr, "ctx2"), (gq2, N * T, "dq2"), (gkv1, N * Rr, "dk1 | dv1"), (gq1, N * Rr, "dq1"),
                            (gkv2, N * T, "dk2 | dv2")):
        _untouched(buf, rows, Hb, set(range(buf.shape[1] // Hb)), what)
    leaves = [t.clone().requires_grad_() for t in (q1, kv1, q2, kv2)]
    c1, c2, l1, l2 = ops.CoAttentionFn.apply(*leaves, m1, m2, N, Rr, T, heads, p, p, rng, 7, 8)
    torch.autograd.backward([c1, c2], [g1, g2])
    a_raw = dict(out=ctx1[:N * T], dq=gq2[:N * T], dk=gkv1[:N * Rr, :Hb], dv=gkv1[:N * Rr, Hb:])
    b_raw = dict(out=ctx2[:N * Rr], dq=gq1[:N * Rr], dk=gkv2[:N * T, :Hb], dv=gkv2[:N * T, Hb:])
    for x, y, what in ((c1.detach(), a_raw["out"], "ctx1"), (c2.detach(), b_raw["out"], "ctx2"), (l1, lse1, "lse1"), (l2, lse2, "lse2"),
                       (leaves[2].grad, a_raw["dq"], "dq2"), (leaves[1].grad[:, :Hb], a_raw["dk"], "dk1"), (leaves[1].grad[:, Hb:], a_raw["dv"], "dv1"),
                       (leaves[0].grad, b_raw["dq"], "dq1"), (leaves[3].grad[:, :Hb], b_raw["dk"], "dk2"), (leaves[3].grad[:, Hb:], b_raw["dv"], "dv2")):
        assert torch.equal(x, y), (what, float((x - y).abs().max()))
    a = _collect(a_raw, (q2, kv1[:, :Hb], kv1[:, Hb:], g1), N, heads, d, T, Rr)
    b = _collect(b_raw, (q1, kv2[:, :Hb], kv2[:, Hb:], g2), N, heads, d, Rr, T)
    a["lse"], b["lse"] = lse1, lse2
    keep_a = keep_b = None
    if p > 0:
        keep_a = F.recover_keep(ops._attn_fwd, dev, F32, N, heads, d, T, Rr, p, rng, 7)
        keep_b = F.recover_keep(ops._attn_fwd, dev, F32, N, heads, d, Rr, T, p, rng, 8)
    _hold(f"pair R{Rr} T{T} d{d} p{p} text-over-regions", form, a, m1, None, keep_a, p, d, share=False)
    _hold(f"pair R{Rr} T{T} d{d} p{p} regions-over-text", form, b, m2, None, keep_b, p, d, share=False)


# ---- E: bias forms ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["default", "two_wave"], indirect=True)
@pytest.mark.parametrize("bform", ["nh", "n1T"])
@pytest.mark.parametrize("N,heads,d,Tq,Tk", F.SHAPES_BIAS)
def test_bias_forms(dev, lib, form, N, heads, d, Tq, Tk, bform):
    """A per-score bias ([N, heads, Tq, Tk] and the transposed view of [N, 1, Tk, Tq]) with its -10000 and -inf entries left in, plus one key whose
    whole column is -inf in one plane: its dk and dv rows depend on nothing but zeros of dS and P and must be exactly zero."""
    A, B, dout = (t.to(dev) for t in F.packed_inputs_f32(N, heads, d, Tq, Tk))
    mask = F.make_mask(N, Tk, "tail").to(dev)
    bias, _ = make_bias(dev, bform, N, heads, Tq, Tk)
    dense = F.with_inf_column(bias).double().expand(N, heads, Tq, Tk)
    run = _launch(dev, A, F.Q_OFF, B, F.K_OFF, B, F.V_OFF, dout, mask, N, heads, d, Tq, Tk, bias=bias)
    exact, _ = _hold(f"bias {bform} N{N} h{heads} d{d} Tq{Tq} Tk{Tk}", form, run, mask, dense, None, 0.0, d)
    assert bool(torch.isinf(dense).any()) and float(exact["dS"][torch.isinf(dense)].abs().max()) == 0
    hs = range(heads) if bform == "n1T" else [heads - 1]
    for h in hs:
        assert float(exact["dk"][0, h, F.INF_KEY].abs().max()) == 0 and float(exact["dv"][0, h, F.INF_KEY].abs().max()) == 0
        assert float(run["got"]["dk"][0, h, F.INF_KEY].abs().max()) == 0 and float(run["got"]["dv"][0, h, F.INF_KEY].abs().max()) == 0


# ---- F: layout independence ---------------------------------------------------------------------------------------------------------------------
def test_packed_and_separate_operands_give_the_same_bits(dev, lib):
    N, heads, d, Tq, Tk = 2, 2, 64, 33, 65
    H = heads * d
    A, B, dout = (t.to(dev) for t in F.packed_inputs_f32(N, heads, d, Tq, Tk))
    mask = F.make_mask(N, Tk, "tail").to(dev)
    packed = _launch(dev, A, F.Q_OFF, B, F.K_OFF, B, F.V_OFF, dout, mask, N, heads, d, Tq, Tk)
    q, k, v = (t[:, b * H:(b + 1) * H].contiguous() for t, b in ((A, F.Q_OFF), (B, F.K_OFF), (B, F.V_OFF)))
    separate = _launch(dev, q, 0, k, 0, v, 0, dout, mask, N, heads, d, Tq, Tk)
    assert torch.equal(packed["lse"], separate["lse"])
    for name in F.OUTPUTS:
        assert torch.equal(packed["raw"][name], separate["raw"][name]), name
