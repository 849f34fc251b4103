"""GPU: global gradient-norm clipping fused into the arena AdamW step (AdamW.max_grad_norm / skip_nonfinite; ytvln_grad_sumsq ->
ytvln_grad_clip_coef -> ytvln_adamw_clip).

Bars and where they come from:
  * norm, relative 1e-5.  A record of a chunk table holds at most CHUNK = 16384 elements: a thread of the 256-thread workgroup adds at
    most 64 squares serially into one fp32 accumulator (each an fma: the square itself is not rounded), then the fixed tree adds 8 levels
    (6 in the wave, 2 across the 4 waves): a chain of <= 72 roundings, plus the fp32 rounding of each partial's use -- <= 73 * 2^-24
    = 4.4e-6 on the sum of squares in the worst case, half that on its root; the partials are summed in fp64.  Every record of every table
    in this file is <= CHUNK long, as every record the optimizer builds.
  * coefficient: the norm's bar plus four fp32 roundings (norm to fp32, the + 1e-6, the division, the product with grad_scale).
  * parameters after clipped steps against the oracle: the project's fp32 bars -- element-wise 2e-6 + 2e-5 |ref| (g0), norms 2e-6 relative.
  * everything called bit-identical is compared with torch.equal on the bits."""
import math
import os
import struct
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT
from helpers import ZERO_DROP, args_ns, cfg_dict, close
from test_rccl_gpu import _batch, _build, _flat, _free_port

pytestmark = pytest.mark.gpu

CHUNK = 16384
NORM_RTOL = 1e-5
COEF_RTOL = NORM_RTOL + 4 * 2.0 ** -24
MAX_NORM = 0.01          # far below the gradient norm of the micro model's first steps (asserted where it is used)


def _table(records, dev, wd=0.0):
    rec = b"".join(struct.pack("<qqff", o, n, wd, 0.0) for o, n in records)
    return torch.frombuffer(bytearray(rec), dtype=torch.uint8).to(dev), len(records)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _norm_of(g, table, nrec, scale, max_norm=math.inf, skip=False, clip=None):
    from ytvln import ops
    partials = torch.full((nrec + 3,), 7.0, dtype=torch.float32, device=g.device)          # (three spare slots must stay untouched)
    clip = torch.zeros(4, dtype=torch.float32, device=g.device) if clip is None else clip
    ops.grad_sumsq(g, table, nrec, partials)
    ops.grad_clip_coef(partials, nrec, scale, max_norm, skip, clip)
    torch.cuda.synchronize()
    assert (partials[nrec:] == 7.0).all()
    return partials, clip


# ---- norm ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_norm_of_odd_records_matches_fp64(dev, lib, dtype, scale):
    n = 3 * CHUNK + 16000
    gen = torch.Generator().manual_seed(7)
    g = (torch.randn(n, generator=gen) * torch.exp2(torch.randint(-6, 6, (n,), generator=gen).float())).to(dtype).to(dev)
    # AdamW-like records (offsets multiples of 4, odd lengths: scalar tails), a single element, a misaligned record (all scalar), gaps
    records = [(0, CHUNK), (CHUNK + 4, 1001), (CHUNK + 1012, 7), (CHUNK + 1024, 1), (CHUNK + 1028, 3), (CHUNK + 2000, CHUNK),
               (2 * CHUNK + 4000, CHUNK - 1), (2 * CHUNK + 2001, 13), (3 * CHUNK + 4000, 11997)]
    covered = torch.zeros(n, dtype=torch.bool)
    for o, l in records:
        assert 0 <= o and o + l <= n and l <= CHUNK and not covered[o:o + l].any()
        covered[o:o + l] = True
    table, nrec = _table(records, dev)
    partials, clip = _norm_of(g, table, nrec, scale)
    gd = g.double()
    for i, (o, l) in enumerate(records):
        want = float((gd[o:o + l] ** 2).sum())
        assert abs(float(partials[i]) - want) <= 2 * NORM_RTOL * want, (i, float(partials[i]), want)
    want = math.sqrt(float((gd[covered.to(dev)] ** 2).sum())) * scale
    got = float(clip[0])
    print(f"norm {dtype} scale {scale}: got {got!r} want {want!r} rel {abs(got - want) / want:.3e}")
    assert abs(got - want) <= NORM_RTOL * want
    assert clip.tolist()[1:] == [1.0, 0.0, 0.0]
    partials2, clip2 = _norm_of(g, table, nrec, scale)
    assert torch.equal(_bits(partials), _bits(partials2)) and torch.equal(_bits(clip), _bits(clip2)), "two runs must be bit-equal"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_norm_of_a_50m_element_arena_matches_fp64(dev, lib, dtype):
    n = 50_000_003                                                   # 3052 records, the last one 11779 long (a scalar tail of 3)
    g = torch.empty(n, dtype=torch.float32, device=dev).normal_(generator=torch.Generator(device=dev).manual_seed(3)).to(dtype)
    records = [(o, min(CHUNK, n - o)) for o in range(0, n, CHUNK)]
    table, nrec = _table(records, dev)
    partials, clip = _norm_of(g, table, nrec, 0.25)
    want = math.sqrt(float((g.double() ** 2).sum())) * 0.25
    got = float(clip[0])
    print(f"norm 50M {dtype}: got {got!r} want {want!r} rel {abs(got - want) / want:.3e}")
    assert abs(got - want) <= NORM_RTOL * want
    partials2, clip2 = _norm_of(g, table, nrec, 0.25)
    assert torch.equal(_bits(partials), _bits(partials2)) and torch.equal(_bits(clip), _bits(clip2)), "two runs must be bit-equal"


def test_empty_inputs(dev, lib):
    from ytvln import ops
    clip = torch.tensor([5.0, 5.0, 5.0, 2.0], device=dev)
    ops.grad_clip_coef(torch.zeros(4, device=dev), 0, 1.0, 1.0, True, clip)
    torch.cuda.synchronize()
    assert clip.tolist() == [0.0, 1.0, 0.0, 2.0]                     # n == 0: norm 0, coef 1, skip 0; the count is kept
    g = torch.ones(64, device=dev)
    partials = torch.full((4,), 3.0, device=dev)
    ops.grad_sumsq(g, _table([(0, 64)], dev)[0], 0, partials)        # nchunks == 0: nothing is written
    torch.cuda.synchronize()
    assert (partials == 3.0).all()
    with pytest.raises(RuntimeError, match="float32 or bfloat16"):
        ops.grad_sumsq(g.half(), _table([(0, 64)], dev)[0], 1, partials)
    with pytest.raises(RuntimeError, match="max_norm"):
        ops.grad_clip_coef(partials, 1, 1.0, -1.0, False, clip)


# ---- coefficient --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["above", "below", "inf"])
def test_coefficient_matches_torch_clip_grad_norm(dev, lib, which):
    gen = torch.Generator().manual_seed(13)
    shapes = [(300, 70), (70,), (5, 1001), (1,)]
    grads = [torch.randn(s, generator=gen) * 0.3 for s in shapes]
    # fp64 copies on the CPU: torch's own answer without torch's fp32 rounding
    ps = [torch.nn.Parameter(torch.zeros(s, dtype=torch.float64)) for s in shapes]
    for p, gr in zip(ps, grads):
        p.grad = gr.double().clone()
    norm = float(torch.nn.utils.clip_grad_norm_(ps, math.inf))       # (max_norm = inf: measures, scales by 1)
    max_norm = {"above": 0.37 * norm, "below": 2.5 * norm, "inf": math.inf}[which]
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm, error_if_nonfinite=False)
    coef_torch = float(ps[0].grad.reshape(-1)[17] / grads[0].double().reshape(-1)[17])
    # the same values in an arena: slots aligned to 4, CHUNK records
    offs, off = [], 0
    for gr in grads:
        offs.append(off)
        off += (gr.numel() + 3) // 4 * 4
    arena = torch.zeros(off)
    records = []
    for o, gr in zip(offs, grads):
        arena[o:o + gr.numel()] = gr.reshape(-1)
        records += [(o + c, min(CHUNK, gr.numel() - c)) for c in range(0, gr.numel(), CHUNK)]
    table, nrec = _table(records, dev)
    _, clip = _norm_of(arena.to(dev), table, nrec, 1.0, max_norm)
    got_norm, got_coef = float(clip[0]), float(clip[1])
    print(f"{which}: norm {got_norm!r} vs torch {float(total)!r}; coef {got_coef!r} vs torch {coef_torch!r}")
    assert abs(got_norm - float(total)) <= NORM_RTOL * float(total)
    if which == "above":
        assert coef_torch < 1.0 and abs(got_coef - coef_torch) <= COEF_RTOL * coef_torch
    else:
        assert coef_torch == 1.0 and got_coef == 1.0                 # exactly 1: the update is then the unclipped one bit for bit
    assert clip.tolist()[2:] == [0.0, 0.0]


# ---- bit-identity when inactive -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["f32", "bf16copy", "gbf16", "gbf16+copy"])
@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adamw_clip_with_coef_one_equals_the_plain_kernels(dev, lib, form, scale, wd):
    from ytvln import ops
    n = 2 * CHUNK + 5003
    gen = torch.Generator().manual_seed(11)
    p0 = torch.randn(n, generator=gen).to(dev)
    m0 = (0.1 * torch.randn(n, generator=gen)).to(dev)
    v0 = (0.01 * torch.rand(n, generator=gen)).to(dev)
    g = torch.randn(n, generator=gen) * 3
    g = (g.to(torch.bfloat16) if form.startswith("gbf16") else g).to(dev)
    copy = form in ("bf16copy", "gbf16+copy")
    records = [(0, CHUNK), (CHUNK, CHUNK), (2 * CHUNK + 4, 4999)]      # tails; element 2*CHUNK .. +3 not in the table
    table, nrec = _table(records, dev, wd)
    hyper = torch.tensor([0.9, 0.999, 1e-6, 1e-3 * (1 - 0.999 ** 3) ** 0.5 / (1 - 0.9 ** 3), 1e-3, 0, 0, 0], dtype=torch.float32, device=dev)
    clip = torch.tensor([123.0, 1.0, 0.0, 0.0], device=dev)
    outs = []
    for clipped in (False, True):
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        pb = torch.zeros(n, dtype=torch.bfloat16, device=dev) if copy else None
        for _ in range(2):
            if clipped:
                ops.adamw_step_clip(p, g, m, v, table, nrec, hyper, clip, scale, p_bf16=pb)
            elif form.startswith("gbf16"):
                ops.adamw_step_gbf16(p, g, m, v, table, nrec, hyper, scale, p_bf16=pb)
            else:
                ops.adamw_step(p, g, m, v, table, nrec, hyper, scale, p_bf16=pb)
        torch.cuda.synchronize()
        outs.append((p, m, v, pb))
    (p1, m1, v1, pb1), (p2, m2, v2, pb2) = outs
    assert not torch.equal(p1, p0)
    for a, b in ((p1, p2), (m1, m2), (v1, v2)):
        assert torch.equal(_bits(a), _bits(b))
    if copy:
        assert torch.equal(_bits(pb1), _bits(pb2))
    assert clip.tolist() == [123.0, 1.0, 0.0, 0.0]                       # read-only for the update


def _micro(dev, seed=11):
    from test_model_gpu import build_lily
    args = args_ns(ranking=True, traj_judge=True, masked_vision=True, masked_language=True)
    args.learning_rate = 1e-3
    model, W = build_lily(dev, "micro.json", args, seed=seed)
    return model.train(), args, W


def _micro_batch(dev, as_numpy=False):
    from ytvln import synth
    nb = synth.make_batch(bs=2, K=3, T=8, frames=2, boxes=3, F=16, C=11, vocab=97, seed=21, opt_holes=1, ignore_rank_frac=0.0)
    return nb if as_numpy else synth.to_torch(nb, dev)


def _train(dev, steps, max_grad_norm=None, skip_nonfinite=False):
    from ytvln import utils_init as U
    from ytvln.vilbert_init import get_optimization
    model, args, _ = _micro(dev)
    args.max_grad_norm, args.skip_nonfinite_grads = max_grad_norm, skip_nonfinite
    opt, sched, _, _ = get_optimization(args, model, 10, None)
    batch = _micro_batch(dev)
    norms = []
    for i in range(steps):
        U.train_step(model, opt, sched, batch, args, i, all_options=bool(batch[13].all()))
        if opt.clip_settings() is not None:
            norms.append(opt.grad_norm().clone())
    torch.cuda.synchronize()
    return model, opt, [float(x) for x in norms]


def test_training_with_a_huge_max_grad_norm_is_bit_identical_to_none(dev, lib):
    m0, o0, _ = _train(dev, 3)
    m1, o1, norms = _train(dev, 3, max_grad_norm=1e30)
    assert o0._arena["clip"] is None and o0._arena["partials"] is None, "feature off: nothing may be allocated"
    assert o1._arena["clip"] is not None and all(0.0 < x < 1e30 for x in norms)
    assert torch.equal(_bits(o0._arena["p"]), _bits(o1._arena["p"]))
    assert torch.equal(_bits(o0._arena["m"]), _bits(o1._arena["m"])) and torch.equal(_bits(o0._arena["v"]), _bits(o1._arena["v"]))
    assert np.array_equal(_flat(m0), _flat(m1))
    assert o1.skipped_steps() == 0 and o0.skipped_steps() == 0


# ---- clipped update against the oracle --------------------------------------------------------------------------------------------------
def test_three_clipped_steps_match_the_oracle_on_scaled_gradients(dev, lib):
    import vilbert_ref as O
    from ytvln import synth
    from ytvln import utils_init as U
    from ytvln.vilbert_init import get_optimization
    model, args, W = _micro(dev)
    nb = _micro_batch(dev, as_numpy=True)
    batch, obatch = synth.to_torch(nb, dev), synth.to_torch(nb)
    cfg = O.RefConfig(**cfg_dict("micro.json", **ZERO_DROP))
    fl = O.TaskFlags(ranking=True, traj_judge=True, masked_vision=True, masked_language=True)
    S = {k: torch.from_numpy(v).clone() for k, v in W.items()}
    st = O.AdamWState()
    warm, tot = O.schedule_totals(10, 1, 1)

    def oracle_grads():
        Wt = O.trainable(S)
        ids, feat, loc, seg, imask, vmask = O.model_input(obatch)
        out = O.lily_forward(Wt, cfg, fl, ids, feat, loc, seg, imask, vmask)
        loss, _ = O.total_loss(obatch, out, fl)
        loss.backward()
        names = [k for k in Wt if k != "cls.predictions.decoder.weight"]
        return names, {k: Wt[k].grad for k in names}

    def norm64(grads):
        return math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads.values() if g is not None))

    max_norm = 0.5 * norm64(oracle_grads()[1])           # below the measured norm of the first step (and asserted at every step)
    args.max_grad_norm = max_norm
    opt, sched, _, _ = get_optimization(args, model, 10, None)
    for step in range(3):
        names, grads = oracle_grads()
        onorm = norm64(grads)
        coef = min(1.0, max_norm / (onorm + 1e-6))
        assert coef < 1.0, (step, onorm, max_norm)
        scaled = {k: None if g is None else (g.double() * coef).float() for k, g in grads.items()}
        O.adamw_step({k: S[k] for k in names}, scaled, st, 1e-3 * O.warmup_linear(step, warm, tot))
        if "cls.predictions.decoder.weight" in S:
            S["cls.predictions.decoder.weight"] = S["bert.embeddings.word_embeddings.weight"]
        U.train_step(model, opt, sched, batch, args, step, all_options=bool(batch[13].all()))
        got = float(opt.grad_norm())
        print(f"step {step}: grad_norm {got!r} oracle {onorm!r} rel {abs(got - onorm) / onorm:.3e} coef {coef:.6f}")
        assert abs(got - onorm) <= NORM_RTOL * onorm
        assert abs(float(opt._arena["clip"][1]) - coef) <= 2 * COEF_RTOL * coef
    for n, p in model.named_parameters():
        close(p, S[n], 2e-6, 2e-5, "after3/" + n)
        n_ref = float(S[n].double().norm())
        assert abs(float(p.detach().double().norm()) - n_ref) <= 2e-6 * n_ref + 1e-6, f"norm after 3 clipped steps: {n}"
    # and the clipping did something: the unclipped run ends somewhere else
    plain, _, _ = _train(dev, 3)
    assert not np.array_equal(_flat(plain), _flat(model))


# ---- skip -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gdtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_skip_leaves_everything_untouched_and_counts(dev, lib, gdtype, bad):
    from ytvln import ops
    n = 2 * CHUNK + 5003
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(n, generator=gen).to(dev)
    m0 = (0.1 * torch.randn(n, generator=gen)).to(dev)
    v0 = (0.01 * torch.rand(n, generator=gen)).to(dev)
    pb0 = p0.to(torch.bfloat16)
    g = torch.randn(n, generator=gen).to(gdtype).to(dev)
    records = [(0, CHUNK), (CHUNK, CHUNK), (2 * CHUNK, 5003)]
    table, nrec = _table(records, dev, 0.01)
    hyper = torch.tensor([0.9, 0.999, 1e-6, 1e-3, 1e-3, 0, 0, 0], dtype=torch.float32, device=dev)
    p, m, v, pb = p0.clone(), m0.clone(), v0.clone(), pb0.clone()
    clip = torch.zeros(4, device=dev)
    gbad = g.clone()
    gbad[2 * CHUNK + 5001] = bad                                     # written into the arena, in a scalar tail
    _norm_of(gbad, table, nrec, 1.0, 1.0, True, clip)
    ops.adamw_step_clip(p, gbad, m, v, table, nrec, hyper, clip, 1.0, p_bf16=pb)
    torch.cuda.synchronize()
    assert not math.isfinite(float(clip[0])) and clip.tolist()[2:] == [1.0, 1.0]
    for a, b in ((p, p0), (m, m0), (v, v0), (pb, pb0)):
        assert torch.equal(_bits(a), _bits(b)), "a skipped step must leave p, m, v and the bf16 copy bit-unchanged"
    # the next clean step updates normally: the plain kernels' result on the clipped gradient scale, and the count stays
    _norm_of(g, table, nrec, 1.0, 1e30, True, clip)
    ops.adamw_step_clip(p, g, m, v, table, nrec, hyper, clip, 1.0, p_bf16=pb)
    q, qm, qv, qb = p0.clone(), m0.clone(), v0.clone(), pb0.clone()
    (ops.adamw_step_gbf16 if gdtype == torch.bfloat16 else ops.adamw_step)(q, g, qm, qv, table, nrec, hyper, 1.0, p_bf16=qb)
    torch.cuda.synchronize()
    assert clip.tolist()[1:] == [1.0, 0.0, 1.0]
    for a, b in ((p, q), (m, qm), (v, qv), (pb, qb)):
        assert torch.equal(_bits(a), _bits(b))
    assert not torch.equal(p, p0)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_without_skip_a_nonfinite_norm_behaves_as_in_torch(dev, lib, bad):
    """torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False): an infinite norm gives the coefficient 0 (finite gradients become 0, the
    infinite one NaN), a NaN norm the coefficient NaN.  The clip-aware update on the raw gradients must equal the plain update on the
    gradients torch scaled."""
    from ytvln import ops
    n = CHUNK + 1003
    gen = torch.Generator().manual_seed(6)
    p0, m0, v0 = torch.randn(n, generator=gen), 0.1 * torch.randn(n, generator=gen), 0.01 * torch.rand(n, generator=gen)
    g = torch.randn(n, generator=gen)
    g[77] = bad
    tp = torch.nn.Parameter(torch.zeros(n))
    tp.grad = g.clone()
    total = torch.nn.utils.clip_grad_norm_([tp], 1.0, error_if_nonfinite=False)
    table, nrec = _table([(0, CHUNK), (CHUNK, 1003)], dev, 0.01)
    hyper = torch.tensor([0.9, 0.999, 1e-6, 1e-3, 1e-3, 0, 0, 0], dtype=torch.float32, device=dev)
    gd = g.to(dev)
    _, clip = _norm_of(gd, table, nrec, 1.0, 1.0, False)
    got = clip.tolist()
    assert (math.isnan(got[0]) and math.isnan(float(total))) or got[0] == float(total)
    assert (math.isnan(got[1]) if math.isnan(bad) else got[1] == 0.0) and got[2:] == [0.0, 0.0]
    a = [t.clone().to(dev) for t in (p0, m0, v0)]
    b = [t.clone().to(dev) for t in (p0, m0, v0)]
    ops.adamw_step_clip(a[0], gd, a[1], a[2], table, nrec, hyper, clip, 1.0)
    ops.adamw_step(b[0], tp.grad.to(dev), b[1], b[2], table, nrec, hyper, 1.0)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(torch.isnan(x), torch.isnan(y))
        assert torch.equal(_bits(torch.nan_to_num(x)), _bits(torch.nan_to_num(y)))
    assert bool(torch.isnan(a[0]).any())


def test_model_step_with_an_inf_gradient_is_skipped_then_training_goes_on(dev, lib):
    from ytvln import ops
    from ytvln import utils_init as U
    from ytvln.vilbert_init import get_optimization
    ops.set_matmul_precision("bf16")                                 # the bf16-resident path: the optimizer also owns a bf16 weight copy
    try:
        model, args = _build(dev, wide=True)
        args.learning_rate, args.skip_nonfinite_grads = 1e-3, True
        opt, sched, _, _ = get_optimization(args, model, 10, None)
        assert opt.max_grad_norm is None and opt.skip_nonfinite
        batch = _batch(dev)
        for i in range(2):
            U.train_step(model, opt, sched, batch, args, i, all_options=True)
        assert opt.skipped_steps() == 0 and math.isfinite(float(opt.grad_norm()))
        a = opt._arena
        assert a["pb"] is not None
        before = [a[k].clone() for k in ("p", "m", "v", "pb")]
        U.train_step(model, opt, None, batch, args, 2, all_options=True, optimizer_step=False)
        lo, hi = a["g"].data_ptr(), a["g"].data_ptr() + 4 * a["g"].numel()
        victim = next(p for p in model.parameters() if p.grad is not None and lo <= p.grad.data_ptr() < hi)
        o, n = opt.arena_range(victim)
        a["g"][o + n // 2] = float("inf")                            # an inf written into the gradient arena, in a slot backward wrote directly
        opt.step()
        sched.step()
        opt.zero_grad()
        assert opt.skipped_steps() == 1 and float(opt.grad_norm()) == math.inf
        for k, old in zip(("p", "m", "v", "pb"), before):
            assert torch.equal(_bits(a[k]), _bits(old)), k
        assert all(opt.state[p]["step"] == 3 for p in model.parameters() if p in opt.state and "step" in opt.state[p])      # (documented)
        U.train_step(model, opt, sched, batch, args, 3, all_options=True)
        assert opt.skipped_steps() == 1 and math.isfinite(float(opt.grad_norm()))
        assert not torch.equal(a["p"], before[0]) and bool(torch.isfinite(a["p"]).all())
        assert torch.equal(_bits(a["pb"]), _bits(a["p"].to(torch.bfloat16)))
    finally:
        ops.set_matmul_precision("fp32")


# ---- capture ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graph_replay_with_clipping_equals_eager(dev, lib, precision):
    from test_model_gpu import build_lily
    from ytvln import ops, synth
    from ytvln import utils_init as U
    from ytvln.vilbert_init import get_optimization
    args = args_ns(ranking=True, traj_judge=True, masked_vision=True, masked_language=True)
    args.learning_rate, args.max_grad_norm, args.skip_nonfinite_grads = 1e-3, MAX_NORM, True
    if precision == "fp32":
        cfg = "micro.json"
        batch = synth.to_torch(synth.make_batch(bs=2, K=3, T=8, frames=2, boxes=3, F=16, C=11, vocab=97, seed=21, ignore_rank_frac=0.0), dev)
    else:
        cfg = "tiny_2_2_1.json"      # head dimension 64: the bf16-resident attention kernels
        batch = synth.to_torch(synth.make_batch(bs=2, K=7, T=16, frames=2, boxes=4, seed=22, ignore_rank_frac=0.0), dev)
    finals, norms, coefs = [], [], []
    ops.set_matmul_precision(precision)
    try:
        for mode in ("eager", "graph"):
            model, _ = build_lily(dev, cfg, args, seed=11)
            model.train()
            opt, sched, _, _ = get_optimization(args, model, 10, None)
            seen = []
            for i in range(2):
                U.train_step(model, opt, sched, batch, args, i, all_options=True)
            if mode == "eager":
                for i in range(2, 5):
                    U.train_step(model, opt, sched, batch, args, i, all_options=True)
                    seen.append(opt._arena["clip"].clone())
            else:
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    U.train_step(model, opt, None, batch, args, 0, all_options=True)
                for i in range(2, 5):
                    opt.prepare_replay()
                    g.replay()
                    sched.step()
                    seen.append(opt._arena["clip"].clone())
                opt.max_grad_norm = 2 * MAX_NORM                      # changed after the capture: the next replay path refuses
                with pytest.raises(RuntimeError, match="capture the step again"):
                    opt.prepare_replay()
                opt.max_grad_norm = MAX_NORM
                opt.prepare_replay()
            torch.cuda.synchronize()
            finals.append((opt._arena["p"].clone(), opt._arena["m"].clone(), opt._arena["v"].clone()))
            norms.append([float(c[0]) for c in seen])
            coefs.append([float(c[1]) for c in seen])
    finally:
        ops.set_matmul_precision("fp32")
    print("norms", norms, "coefs", coefs)
    assert norms[0] == norms[1] and coefs[0] == coefs[1]
    assert len(set(norms[1])) == 3, "the norm must be computed inside the graph, not baked in"
    assert all(c < 1.0 for c in coefs[1]), "the clipping must be active in this test"
    for a, b in zip(finals[0], finals[1]):
        assert torch.equal(_bits(a), _bits(b)), float((a - b).abs().max())


# ---- data parallel on one GPU -------------------------------------------------------------------------------------------------------------
def _fwd_bwd(U, dp, opt, batch, args):
    return lambda backward=None: U.train_step(dp, opt, None, batch, args, 0, all_options=True, optimizer_step=False, backward=backward)[0]


def _plain_clipped_run(dev, precision="fp32", steps=3, rounded=False):
    """The plain single-process run with clipping on; `rounded`: the gradient arena rounded to bf16 in place before every update (what the
    one-rank bf16 exchange amounts to)."""
    from ytvln import ops, utils_init as U
    from ytvln.vilbert_init import get_optimization
    ops.set_matmul_precision(precision)
    try:
        model, args = _build(dev, wide=precision != "fp32")
        args.learning_rate, args.max_grad_norm = 1e-3, MAX_NORM
        opt, sched, _, _ = get_optimization(args, model, 10, None)
        if rounded:
            opt.grad_sync = lambda flat, layout: flat.copy_(flat.bfloat16().float())
        batch = _batch(dev)
        clips = []
        for step in range(steps):
            U.train_step(model, opt, sched, batch, args, step, all_options=True)
            clips.append(opt._arena["clip"].clone())
        torch.cuda.synchronize()
        return _flat(model), [c.tolist() for c in clips]
    finally:
        ops.set_matmul_precision("fp32")


def _one_rank_worker(case, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                          HSA_ENABLE_IPC_MODE_LEGACY="0")
        os.environ.pop("YTVLN_DP_GRAD_DTYPE", None)
        sys.path.insert(0, os.path.join(ROOT, "youtube-vln_amd"))
        import torch.distributed as dist
        from ytvln import distributed as D, ops, utils_init as U
        from ytvln.vilbert_init import get_optimization
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(0)
        case, _, precision = case.partition("@")
        ops.set_matmul_precision(precision or "fp32")
        mode, _, gdtype = case.partition("/")
        D.init_distributed(backend="gloo", force=True)
        model, args = _build(dev, wide=bool(precision))
        args.learning_rate, args.max_grad_norm = 1e-3, MAX_NORM
        dp = D.DataParallel(model, bucket_bytes=64 << 10, collective="rccl", always_exchange=True, grad_dtype=gdtype or "fp32")
        opt, sched, _, _ = get_optimization(args, model, 10, None)
        dp.attach(opt)
        batch = _batch(dev)
        clips = []
        if mode == "eager":
            for step in range(3):
                U.train_step(dp, opt, sched, batch, args, step, all_options=True)
                clips.append(opt._arena["clip"].clone())
        else:
            U.train_step(dp, opt, sched, batch, args, 0, all_options=True)
            clips.append(opt._arena["clip"].clone())
            gs = D.GraphedTrainStep(dp, opt, _fwd_bwd(U, dp, opt, batch, args), bucket_bytes=64 << 10, mode=mode)
            assert gs.mode == mode and gs.exchange
            for _ in range(2):
                gs.step(sched)
                clips.append(opt._arena["clip"].clone())
            if mode == "phased":
                assert len([g for g in gs._group_slices if g]) > 1, "several groups: the update really was deferred past the first ones"
        torch.cuda.synchronize()
        dp.comm.check_async_error()
        norm64 = None
        if gdtype == "bf16":          # the reported norm is that of the bf16 buffer the update read (grad_scale 1 in a one-rank world)
            norm64 = math.sqrt(float((opt.grad_bf16().double() ** 2).sum()))
        out = (_flat(model), [c.tolist() for c in clips], norm64)
        dp.close()
        dist.destroy_process_group()
        q.put(("ok", out))
    except Exception as e:      # surface the failure in the parent instead of a bare exit code
        import traceback
        q.put(("error", traceback.format_exc()))
        raise e


@pytest.mark.parametrize("case", ["eager", "split", "single", "phased", "phased@bf16", "eager/bf16", "split/bf16", "single/bf16", "phased/bf16"])
def test_one_rank_world_with_clipping_equals_the_plain_clipped_run(dev, lib, case):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_one_rank_worker, args=(case, _free_port(), q))
    p.start()
    status, out = q.get(timeout=900)
    p.join(timeout=120)
    assert status == "ok", out
    assert p.exitcode == 0
    got, clips, norm64 = out
    base, _, precision = case.partition("@")
    bf16x = base.endswith("/bf16")
    ref, ref_clips = _plain_clipped_run(dev, precision or "fp32", rounded=bf16x)
    print(case, "clip records", clips, "plain", ref_clips)
    assert all(c[1] < 1.0 and c[2] == 0.0 for c in ref_clips), "the clipping must be active in this test"
    assert clips == ref_clips, "norm and coefficient of every step must not depend on the step form"
    assert np.array_equal(got, ref), float(np.abs(got - ref).max())
    if bf16x:
        assert abs(clips[-1][0] - norm64) <= NORM_RTOL * norm64, (clips[-1][0], norm64)
        plain32, _ = _plain_clipped_run(dev, "fp32")
        assert not np.array_equal(got, plain32), "the bf16 exchange rounds: it cannot equal the fp32 run"


def _two_rank_worker(rank, world, port, q, mode):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                          HSA_ENABLE_IPC_MODE_LEGACY="0")
        os.environ.pop("YTVLN_DP_GRAD_DTYPE", None)
        sys.path.insert(0, os.path.join(ROOT, "youtube-vln_amd"))
        import torch.distributed as dist
        from test_dp_gpu import _batch as _rank_batch, _build as _dp_build
        from ytvln import distributed as D, utils_init as U
        from ytvln.vilbert_init import get_optimization
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(0)
        D.init_distributed(backend="gloo")
        model, args = _dp_build(dev)
        args.learning_rate, args.max_grad_norm = 1e-3, MAX_NORM
        dp = D.DataParallel(model, bucket_bytes=64 << 10, collective="torch")      # two ranks on ONE device: RCCL refuses, gloo carries it
        opt, sched, _, _ = get_optimization(args, model, 10, None)
        dp.attach(opt)
        assert opt.grad_scale == 0.5
        batch = _rank_batch(rank, dev)
        norms = []
        if mode == "eager":
            for step in range(3):
                U.train_step(dp, opt, sched, batch, args, step, all_options=True)
                norms.append(float(opt.grad_norm()))
        else:
            U.train_step(dp, opt, sched, batch, args, 0, all_options=True)
            norms.append(float(opt.grad_norm()))
            if mode == "phased":
                os.environ["YTVLN_DP_CUTS"] = "t0,c0,v1"
            gs = D.GraphedTrainStep(dp, opt, _fwd_bwd(U, dp, opt, batch, args), bucket_bytes=64 << 10, mode="phased" if mode == "phased" else None)
            assert gs.mode == ("phased" if mode == "phased" else "split")
            for _ in range(2):
                gs.step(sched)
                norms.append(float(opt.grad_norm()))
        torch.cuda.synchronize()
        flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu()
        both = [torch.zeros_like(flat) for _ in range(world)]
        dist.all_gather(both, flat)
        assert torch.equal(both[0], both[1]), "replicas diverged"
        every = [None] * world
        dist.all_gather_object(every, norms)
        assert every[0] == every[1], f"the ranks report different norms: {every}"
        dist.destroy_process_group()
        q.put((rank, "ok", (flat.numpy(), norms) if rank == 0 else None))
    except Exception as e:
        import traceback
        q.put((rank, "error", traceback.format_exc()))
        raise e


@pytest.mark.parametrize("mode", ["eager", "graphed", "phased"])
def test_two_gloo_ranks_with_clipping_match_the_single_process_average(dev, lib, mode):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_two_rank_worker, args=(r, 2, port, q, mode)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict((r, (s, x)) for r, s, x in (q.get(timeout=600) for _ in range(2)))
    for p in procs:
        p.join(timeout=120)
    assert all(s == "ok" for s, _ in got.values()), got
    assert [p.exitcode for p in procs] == [0, 0]
    w, norms = got[0][1]
    # single process: loss = mean of the two ranks' losses  <=>  averaged gradients; the same clipping
    from test_dp_gpu import _batch as _rank_batch, _build as _dp_build
    from ytvln import utils_init as U
    from ytvln.vilbert_init import get_optimization
    model, args = _dp_build(dev)
    args.learning_rate, args.max_grad_norm = 1e-3, MAX_NORM
    opt, sched, _, _ = get_optimization(args, model, 10, None)
    batches = [_rank_batch(r, dev) for r in range(2)]
    ref_norms = []
    for step in range(3):
        total = None
        for b in batches:
            outputs = model(*U.get_model_input(b, all_options=True))
            for task, flag in U.TASKS:
                _, _, l, _ = U.get_loss_correct(b, outputs, task, args, None, True, all_options=True)
                l = 0.5 * (args.traj_loss_scale * l if task == "traj" else l)
                total = l if total is None else total + l
        total.backward()
        opt.step(); sched.step(); opt.zero_grad()
        ref_norms.append(float(opt.grad_norm()))
        assert float(opt._arena["clip"][1]) < 1.0, "the clipping must be active in this test"
    ref = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu().numpy()
    print(mode, "norms", norms, "single process", ref_norms)
    assert np.allclose(got[0][1][0], ref, atol=2e-6, rtol=2e-5), float(np.abs(w - ref).max())
    # the norm of the averaged gradient: two ways of summing the same numbers in fp32 upstream of it (the project's gradient bar is 1e-4)
    assert all(abs(a - b) <= 1e-4 * b for a, b in zip(norms, ref_norms)), (norms, ref_norms)
