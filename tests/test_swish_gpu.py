"""hidden_act = "swish" on the GPU: the stand-alone activation kernels (ytvln_act_fwd_*, the swish case of ytvln_act_bwd_*), ops.linear(...,
"swish") in the three matmul precisions, and the model against the fixtures generated from the reference (tools/gen_golden_swish.py).

Every tolerance is the one an existing test holds the gelu / relu counterpart to (named at each use); each figure is printed before it is
asserted.  swish is unfused by design: the projection is the plain GEMM, the activation a kernel of its own -- the last test guards that
gelu configurations never reach it."""
import json
import math

import numpy as np
import pytest
import torch

from helpers import ZERO_DROP, args_ns, cfg_dict, close, gold, rel_l2
from test_kernels_gpu import rnd
from test_model_gpu import LOSS_TOL, _bf16_check, build_lily, check_summaries, losses_of
from test_swish_cpu import ALL, micro_weights

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SIZES = [0, 1, 3, 4, 5, 1023, 1024 * 1024 + 7]
SWISH = dict(hidden_act="swish", v_hidden_act="swish")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def act_fwd(z, y=None):
    """ytvln_act_fwd_f32 / _bf16 on flat tensors (y = z: in place)."""
    from ytvln import _lib
    y = _nan_like(z) if y is None else y
    _lib.call("ytvln_act_fwd_bf16" if z.dtype == BF else "ytvln_act_fwd_f32", z.data_ptr(), y.data_ptr(), z.numel(), _lib.ACT_SWISH, _stream())
    return y


def act_bwd(dy, z, dz=None):
    from ytvln import _lib
    dz = _nan_like(z) if dz is None else dz
    _lib.call("ytvln_act_bwd_bf16" if z.dtype == BF else "ytvln_act_bwd_f32", dy.data_ptr(), z.data_ptr(), dz.data_ptr(), z.numel(),
              _lib.ACT_SWISH, _stream())
    return dz


def _flat(t, dev):
    """`t` on the device as the head of a slightly larger buffer: an empty tensor still has a real (16-byte aligned) address."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=dev)
    buf[:t.numel()].copy_(t)
    return buf[:t.numel()]


def _nan_like(t):
    return torch.full((t.numel() + 4,), float("nan"), dtype=t.dtype, device=t.device)[:t.numel()]


def off_by_one(t):
    """The same values in a view that starts one element into its buffer (base pointer off the 16-byte grid)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t)
    assert t.numel() == 0 or buf[1:].data_ptr() % 16 != 0          # (an empty tensor has no address at all)
    return buf[1:]


def swish64(z):
    return z * torch.sigmoid(z)


def dswish64(z):
    s = torch.sigmoid(z)
    return s + z * s * (1 - s)


# ------------------------------------------------------------------------------------------------------------------
# 1 / 2: the kernels
# ------------------------------------------------------------------------------------------------------------------
def test_swish_kernels_fp32_kat(dev, lib):
    """act_fwd and the swish act_bwd against the reference's own values (g19_swish_kats) at atol 1e-6 + rtol 1e-6 -- the bar
    test_gelu_kat_and_act_bwd holds gelu to --, every output finite; all sizes, aligned, off-by-one views and in place."""
    k = gold("g19_swish_kats.npz")
    worst = [0.0, 0.0]
    for n in SIZES:
        x = _flat(torch.from_numpy(np.resize(k["swish/x"], n)), dev)
        y_ref, d_ref = np.resize(k["swish/y"], n), np.resize(k["swish/dy"], n)
        g = _flat(torch.randn(n, generator=torch.Generator().manual_seed(n + 1)), dev)
        forms = [("aligned", x, None), ("view+1 -> aligned", off_by_one(x), None), ("view+1 -> view+1", off_by_one(x), off_by_one(torch.zeros_like(x))),
                 ("aligned -> view+1", x, off_by_one(torch.zeros_like(x))), ("in place", _flat(x, dev), "same"), ("in place, view+1", off_by_one(x), "same")]
        for what, z, out in forms:
            keep = z.clone()
            y = act_fwd(z, z if out == "same" else out)
            assert bool(torch.isfinite(y).all()), (n, what)
            worst[0] = max(worst[0], close(y, y_ref, 1e-6, 1e-6, f"act_fwd n={n} {what}"))
            if out != "same":
                assert torch.equal(z, keep), "the input was written"
        for what, z, dy in (("aligned", x, g), ("view+1", off_by_one(x), off_by_one(g)), ("mixed", x, off_by_one(g))) if n else ():
            dz = act_bwd(dy, z, off_by_one(torch.zeros_like(z)) if what == "view+1" else None)
            assert bool(torch.isfinite(dz).all()), (n, what)
            worst[1] = max(worst[1], close(dz, g.double().cpu() * torch.from_numpy(d_ref).double(), 1e-6, 1e-6, f"act_bwd n={n} {what}"))
        if n:      # upstream gradient of ones: the fixture's derivative itself
            close(act_bwd(torch.ones_like(x), x), d_ref, 1e-6, 1e-6, f"swish' n={n}")
    print(f"[swish fp32 KAT] max abs error forward {worst[0]:.3e}, backward {worst[1]:.3e}")
    # the ends of the range, exactly: no inf / inf or 0 * inf anywhere
    x = torch.tensor([-1e4, 1e4, -3e38, 3e38, 0.0, -0.0], device=dev)
    y, d = act_fwd(x).cpu(), act_bwd(torch.ones_like(x), x).cpu()
    assert y.tolist() == [0.0, 1e4, 0.0, float(np.float32(3e38)), 0.0, 0.0] and bool(torch.signbit(y[0])) and bool(torch.signbit(y[2]))
    assert d.tolist() == [0.0, 1.0, 0.0, 1.0, 0.5, 0.5]


def test_swish_kernels_bf16(dev, lib):
    """bf16 forms against the fp64 formula on the bf16-rounded inputs: at most one bf16 rounding of the exact result (2^-8 relative + 1e-30)."""
    k = gold("g19_swish_kats.npz")
    worst = [0.0, 0.0]

    def check(got, ref, what, slot):
        assert got.dtype == BF and bool(torch.isfinite(got.float()).all()), what
        err = (got.double().cpu() - ref).abs()
        bound = 2.0 ** -8 * ref.abs() + 1e-30
        if got.numel():
            worst[slot] = max(worst[slot], float((err / (ref.abs() + 1e-30)).max()))
        assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} outside one bf16 rounding, worst ratio {float((err / bound).max()):.3f}"

    for n in SIZES:
        x = _flat(torch.from_numpy(np.resize(k["swish/x"], n)).to(BF), dev)
        g = _flat(torch.randn(n, generator=torch.Generator().manual_seed(n + 2)).to(BF), dev)
        y_ref, d_ref = swish64(x.double().cpu()), g.double().cpu() * dswish64(x.double().cpu())
        for what, z, out in (("aligned", x, None), ("view+1 -> aligned", off_by_one(x), None), ("view+1 -> view+1", off_by_one(x), off_by_one(torch.zeros_like(x))),
                             ("in place", _flat(x, dev), "same"), ("in place, view+1", off_by_one(x), "same")):
            check(act_fwd(z, z if out == "same" else out), y_ref, f"act_fwd_bf16 n={n} {what}", 0)
        for what, z, dy in (("aligned", x, g), ("view+1", off_by_one(x), off_by_one(g)), ("mixed", x, off_by_one(g))) if n else ():
            check(act_bwd(dy, z), d_ref, f"act_bwd_bf16 n={n} {what}", 1)
    print(f"[swish bf16] max relative error forward {worst[0]:.3e}, backward {worst[1]:.3e} (one rounding = {2.0 ** -8:.3e})")


# ------------------------------------------------------------------------------------------------------------------
# 3: ops.linear(..., "swish")
# ------------------------------------------------------------------------------------------------------------------
SHAPES = [(4480, 768, 3072), (16128, 1024, 1024), (37, 100, 52)]


def _operands(dev, M, K, N):
    """x ~ N(0, 1), W ~ N(0, 1/K) so that the pre-activation is of order one (where swish bends), dy ~ N(0, 1/M) so that the weight and bias
    gradients -- sums over M rows -- are of order one as well: the scale at which the absolute bars below were set for gelu."""
    x, w, b = rnd(dev, M, K, seed=1), rnd(dev, N, K, seed=2, scale=1.0 / math.sqrt(K)), rnd(dev, N, seed=3, scale=0.5)
    dy = rnd(dev, M, N, seed=4, scale=1.0 / math.sqrt(M))
    return x, w, b, dy


def _ref64(x, w, b, dy):
    td = [t.detach().double().requires_grad_(True) for t in (x, w, b)]
    yr = swish64(torch.nn.functional.linear(*td))
    yr.backward(dy.double())
    return yr.detach(), [t.grad for t in td]


@pytest.mark.parametrize("M,K,N", SHAPES)
def test_linear_swish_fp32(dev, lib, M, K, N):
    """Forward and the three gradients against fp64 torch at the tolerances test_gemm_epilogues_and_strides gives the gelu epilogue (2e-4 / 1e-4
    forward, 3e-4 / 2e-4 backward; plus the model tests' per-tensor 1e-4 relative L2); and step 1 really is the plain GEMM: the result
    equals act_fwd(ops.linear(x, W, b)) bit for bit, with and without a backward to keep z for, and through linear_res."""
    from ytvln import ops
    x, w, b, dy = _operands(dev, M, K, N)
    ts = [t.clone().requires_grad_(True) for t in (x, w, b)]
    y = ops.linear(ts[0], ts[1], ts[2], "swish")
    y.backward(dy)
    yr, gr = _ref64(x, w, b, dy)
    print(f"[linear swish fp32 {M}x{K}->{N}] forward max abs {float((y.detach().double() - yr).abs().max()):.3e}, rel-L2 "
          + ", ".join(f"d{n} {rel_l2(t.grad, r):.2e}" for n, t, r in zip("xwb", ts, gr)))
    close(y, yr, 2e-4, 1e-4, "swish forward")
    for n, t, r in zip("xwb", ts, gr):
        close(t.grad, r, 3e-4, 2e-4, "swish d" + n)
        assert rel_l2(t.grad, r) < 1e-4, n
    with torch.no_grad():
        z = ops.linear(x, w, b)
        y_nograd = ops.linear(x, w, b, "swish")          # in place over z
    want = act_fwd(z.reshape(-1).clone()).view(M, N)
    assert torch.equal(y.detach(), want) and torch.equal(y_nograd, want)
    y2, res = ops.linear_res(ts[0], ts[1], ts[2], "swish")
    assert torch.equal(y2.detach(), want) and res.data_ptr() == ts[0].data_ptr() and res.shape == ts[0].shape


@pytest.mark.parametrize("M,K,N", SHAPES)
def test_linear_swish_bf16(dev, lib, M, K, N):
    """bf16-resident path: against fp64 on the bf16-rounded operands at the bars of the gelu counterparts -- output within 6e-3 of the largest
    entry (test_gemm_bf16_epilogues_splitk_and_padding), gradients within 1e-2 relative L2 (test_linear_ffn_bf16_autograd_and_weight_copies)."""
    from ytvln import ops
    x, w, b, dy = _operands(dev, M, K, N)
    xb = x.to(BF).requires_grad_(True)
    wp, bp = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = ops.linear(xb, wp, bp, "swish")
    assert y.dtype == BF
    dyb = dy.to(BF)
    y.backward(dyb)
    yr, gr = _ref64(xb.detach(), w.to(BF), b, dyb)
    relmax = float((y.double() - yr).abs().max()) / float(yr.abs().max())
    rels = [rel_l2(t.grad, r) for t, r in zip((xb, wp, bp), gr)]
    print(f"[linear swish bf16 {M}x{K}->{N}] forward rel-max {relmax:.3e}, gradient rel-L2 {rels}")
    assert relmax < 6e-3
    assert xb.grad.dtype == BF and wp.grad.dtype == torch.float32 and bp.grad.dtype == torch.float32
    assert all(r < 1e-2 for r in rels), rels
    with torch.no_grad():
        assert torch.equal(ops.linear(xb, wp, bp, "swish"), y.detach())          # in place over z: the same bits
        out32 = ops.linear(xb, wp, bp, "swish", out_fp32=True)
    assert out32.dtype == torch.float32 and torch.equal(out32, y.detach().float())


@pytest.mark.parametrize("M,K,N", SHAPES)
def test_linear_swish_fp32x3(dev, lib, M, K, N):
    """fp32x3 projections: the bars of test_gemm_fp32_split_bf16x3 (max error within 4e-6 * sqrt(K) * 4 + 1e-5 and within twice the native
    kernel's own error + 1e-6; not the native kernel's bits where the split path exists), and the fp32 bars of test_linear_swish_fp32."""
    from ytvln import ops
    x, w, b, dy = _operands(dev, M, K, N)
    yr, gr = _ref64(x, w, b, dy)
    outs, grads = {}, {}
    for mode in ("fp32", "fp32x3"):
        ts = [t.clone().requires_grad_(True) for t in (x, w, b)]
        ops.set_matmul_precision(mode)
        try:
            y = ops.linear(ts[0], ts[1], ts[2], "swish")
            y.backward(dy)
        finally:
            ops.set_matmul_precision("fp32")
        outs[mode], grads[mode] = y.detach(), [t.grad for t in ts]
    e_native, e_split = (float((outs[m].double() - yr).abs().max()) for m in ("fp32", "fp32x3"))
    print(f"[linear swish fp32x3 {M}x{K}->{N}] forward max abs: native {e_native:.3e}, split {e_split:.3e}")
    assert e_split < 4e-6 * math.sqrt(K) * 4.0 + 1e-5 and e_split < 2.0 * e_native + 1e-6, (e_split, e_native)
    if K % 32 == 0:          # (the ragged shape runs on the generic kernel, which ignores the split flag)
        assert not torch.equal(outs["fp32"], outs["fp32x3"]), "fp32x3 reproduced the native kernel bit for bit: the split path did not run"
    close(outs["fp32x3"], yr, 2e-4, 1e-4, "swish forward")
    for n, t, r in zip("xwb", grads["fp32x3"], gr):
        close(t, r, 3e-4, 2e-4, "swish d" + n)
        assert rel_l2(t, r) < 1e-4, n


# ------------------------------------------------------------------------------------------------------------------
# 4 / 5: the model against the reference
# ------------------------------------------------------------------------------------------------------------------
def _micro(dev, g, **acts):
    from ytvln import synth
    args = args_ns(**ALL)
    model, W = build_lily(dev, "micro.json", args, seed=11, **acts)
    Wg = micro_weights(g)
    assert all(np.array_equal(W[k], Wg[k]) for k in W)
    nb = synth.make_batch(bs=2, K=3, T=8, frames=2, boxes=3, F=16, C=11, vocab=97, seed=21, opt_holes=1, ignore_rank_frac=0.0)
    for i, a in enumerate(nb):
        assert np.array_equal(a, g["in_%02d" % i]), f"batch recipe drifted at index {i}"
    return model, args, synth.to_torch(nb, dev)


def _check_forward_and_grads(model, args, batch, g, prefix):
    model.eval()
    with torch.no_grad():
        outputs, total, per = losses_of(model, batch, args)
    for k in ("ranking", "traj", "vision", "language"):
        close(outputs[k], g[prefix + "logits/" + k], 1e-4, 1e-4, prefix + "logits/" + k)
        close(per[k], g[prefix + "loss/" + k], LOSS_TOL, 0, prefix + "loss/" + k)
        close(per["correct_" + k], g[prefix + "loss/correct_" + k], 1e-6, 0, prefix + "correct/" + k)
    close(total, g[prefix + "loss/total"], LOSS_TOL, 0, prefix + "loss/total")


def _check_grads(model, g, prefix):
    assert {n for n, p in model.named_parameters() if p.grad is None} == set(g["unused"].tolist())
    worst = 0.0
    for n, p in model.named_parameters():
        if p.grad is not None:
            ref = g[prefix + "grad/" + n]
            r = rel_l2(p.grad, ref)
            assert r < 1e-4 or float(np.linalg.norm(ref)) < 1e-7, f"{prefix}grad {n}: {r:.2e}"
            if float(np.linalg.norm(ref)) >= 1e-7:
                worst = max(worst, r)
    return worst


def test_g19_swish_micro_everything(dev, lib):
    """The all-swish micro fixture through Lily exactly as test_g0_micro_everything does, at its bars: losses 1e-4, logits 1e-4 / 1e-4,
    per-tensor gradient rel-L2 1e-4 (tiny-norm guard), parameters after three AdamW steps 2e-6 / 2e-5, exp_avg 1e-4, exp_avg_sq 2e-4."""
    from ytvln.vilbert_init import get_optimization
    g, gm = gold("g19_swish_micro.npz"), gold("g19_swish_micro_adamw.npz")
    model, args, batch = _micro(dev, g, **SWISH)
    _check_forward_and_grads(model, args, batch, g, "")
    model.train()
    args.learning_rate = 1e-3
    opt, sched, _, _ = get_optimization(args, model, 10, None)
    for step in range(3):
        outputs, total, per = losses_of(model, batch, args)
        total.backward()
        if step == 0:
            print(f"[g19 swish micro fp32] worst gradient rel-L2 {_check_grads(model, g, ''):.2e}")
        close(total, g[f"step{step}.loss"], LOSS_TOL, 0, f"step{step}.loss")
        assert abs(sched.get_last_lr()[0] - float(g[f"step{step}.lr"])) < 1e-12
        opt.step(); sched.step(); opt.zero_grad()
    for n, p in model.named_parameters():
        close(p, g["after3/" + n], 2e-6, 2e-5, "after3/" + n)
        if ("exp_avg/" + n) in gm.files:
            assert rel_l2(opt.state[p]["exp_avg"], gm["exp_avg/" + n]) < 1e-4 or float(np.linalg.norm(gm["exp_avg/" + n])) < 1e-7, n
            assert rel_l2(opt.state[p]["exp_avg_sq"], gm["exp_avg_sq/" + n]) < 2e-4 or float(np.linalg.norm(gm["exp_avg_sq/" + n])) < 1e-13, n
        else:
            assert p not in opt.state or "exp_avg" not in opt.state[p], n


def test_g19_mixed_swish_text_gelu_image(dev, lib):
    """hidden_act = "swish", v_hidden_act = "gelu": the image stream runs the fused gelu, the text stream and BOTH prediction heads swish (the
    reference's image head applies hidden_act) -- a head built from the wrong field misses the vision logits by far more than 1e-4."""
    g = gold("g19_swish_micro.npz")
    model, args, batch = _micro(dev, g, hidden_act="swish", v_hidden_act="gelu")
    assert model.cls.imagePredictions.transform.transform_act_fn == "swish"
    _check_forward_and_grads(model, args, batch, g, "mixed/")
    model.train()
    outputs, total, per = losses_of(model, batch, args)
    total.backward()
    print(f"[g19 mixed] worst gradient rel-L2 {_check_grads(model, g, 'mixed/'):.2e}")


def test_g19_swish_micro_fp32x3(dev, lib):
    """fp32x3 projections meet the fp32 bars on the swish fixture (as test_fp32x3_meets_the_fp32_bar_on_every_golden does for g0)."""
    from ytvln import ops
    ops.set_matmul_precision("fp32x3")
    try:
        test_g19_swish_micro_everything(dev, lib)
    finally:
        ops.set_matmul_precision("fp32")


def _tiny(dev):
    from ytvln import synth
    args = args_ns(**ALL)
    model, W = build_lily(dev, "tiny_2_2_1.json", args, seed=12, **SWISH)
    batch = synth.to_torch(synth.make_batch(bs=2, K=7, T=16, frames=2, boxes=4, seed=22, ignore_rank_frac=0.0), dev)
    return model, W, args, batch


@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
def test_g19_swish_tiny_summaries(dev, lib, precision):
    """The tiny-config swish fixture at the bars of test_g1 / test_g2 (check_summaries: losses 1e-4, logits 1e-4 / 1e-4, gradient norms
    2e-4, post-AdamW checksums), native fp32 and fp32x3."""
    from ytvln import ops
    g = gold("g19_swish_tiny.npz")
    model, W, args, batch = _tiny(dev)
    ops.set_matmul_precision(precision)
    try:
        check_summaries(model, W, batch, args, g, float(g["lr"]))
    finally:
        ops.set_matmul_precision("fp32")


def test_g19_swish_bf16_resident(dev, lib):
    """The bf16-resident path with swish at the bars of test_g2_full_model_bf16_projections (_bf16_check: every loss within 2e-2 relative,
    gradient norms within 5 % + 1e-4, never the fp32 bits).  It runs on the tiny-config fixture: the bf16-resident attention kernels are
    built for head dimensions 64 and 128 and refuse the micro config's 8 with any activation, which the second half pins."""
    from ytvln import ops
    g = gold("g19_swish_tiny.npz")
    model, W, args, batch = _tiny(dev)
    _bf16_check(model, batch, args, g)
    gm = gold("g19_swish_micro.npz")
    model, args, batch = _micro(dev, gm, **SWISH)
    ops.set_matmul_precision("bf16")
    try:
        with pytest.raises(NotImplementedError, match="head dimensions 64 and 128"):
            losses_of(model, batch, args)
    finally:
        ops.set_matmul_precision("fp32")


# ------------------------------------------------------------------------------------------------------------------
# 6 / 7: training-loop properties keep holding with swish
# ------------------------------------------------------------------------------------------------------------------
def test_loss_aware_heads_match_full_heads_with_swish(dev, lib):
    """test_loss_aware_heads_match_full_heads on a swish model: the row-subset heads go through the same ops.linear."""
    from ytvln import synth
    from ytvln import utils_init as U
    from ytvln.vilbert_init import get_optimization
    args = args_ns(**ALL)
    args.learning_rate = 1e-3
    batch = synth.to_torch(synth.make_batch(bs=3, K=3, T=16, frames=2, boxes=5, F=16, C=11, vocab=97, seed=33, ignore_rank_frac=0.0), dev)
    finals, losses = [], []
    for aware in (False, True):
        model, _ = build_lily(dev, "micro.json", args, seed=5, **SWISH)
        model.train()
        opt, sched, _, _ = get_optimization(args, model, 10, None)
        for i in range(3):
            loss, metrics = U.train_step(model, opt, sched, batch, args, i, all_options=True, loss_aware_heads=aware, capacity_frac=0.5)
        if aware:
            assert float(metrics["head_row_overflow"]) == 0.0
        torch.cuda.synchronize()
        finals.append(torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu())
        losses.append((float(loss), {k: float(v) for k, v in metrics["loss"].items()}))
    assert abs(losses[0][0] - losses[1][0]) < 2e-6 * max(1.0, abs(losses[0][0])), losses
    for k in losses[0][1]:
        assert abs(losses[0][1][k] - losses[1][1][k]) < 2e-6 * max(1.0, abs(losses[0][1][k])), (k, losses)
    assert float((finals[0] - finals[1]).abs().max()) < 5e-6, float((finals[0] - finals[1]).abs().max())


DROPOUT = dict(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, v_attention_probs_dropout_prob=0.1, v_hidden_dropout_prob=0.1)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_swish_graph_replay_and_two_stream_are_bit_identical(dev, lib, precision):
    """test_graph_replay_equals_eager and test_two_stream_equals_one_stream on a swish model in train mode with dropout p = 0.1: five steps
    as eager launches and as a captured, replayed hipGraph, on one stream and on two -- the same parameters and loss BIT FOR BIT (the
    activation kernel allocates like the gelu path and runs on the current stream)."""
    from ytvln import ops, synth
    from ytvln import utils_init as U
    from ytvln.vilbert_init import get_optimization
    args = args_ns(**ALL)
    args.learning_rate = 1e-3
    if precision == "fp32":
        cfg = "micro.json"
        batch = synth.to_torch(synth.make_batch(bs=2, K=3, T=8, frames=2, boxes=3, F=16, C=11, vocab=97, seed=21, ignore_rank_frac=0.0), dev)
    else:
        cfg = "tiny_2_2_1.json"      # head dimension 64: the bf16-resident attention kernels
        batch = synth.to_torch(synth.make_batch(bs=2, K=7, T=16, frames=2, boxes=4, seed=22, ignore_rank_frac=0.0), dev)
    finals, losses = {}, {}
    ops.set_matmul_precision(precision)
    try:
        for two in (False, True):
            for mode in ("eager", "graph"):
                ops.set_two_stream(two)
                ops.DropoutState.manual_seed(1234)
                model, _ = build_lily(dev, cfg, args, seed=11, dropout=0.1, **SWISH, **DROPOUT)
                model.train()
                opt, sched, _, _ = get_optimization(args, model, 10, None)
                for i in range(2):
                    U.train_step(model, opt, sched, batch, args, i, all_options=True)
                if mode == "eager":
                    for i in range(2, 5):
                        loss, _ = U.train_step(model, opt, sched, batch, args, i, all_options=True)
                else:
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        loss, _ = U.train_step(model, opt, None, batch, args, 0, all_options=True)
                    for i in range(2, 5):
                        opt.prepare_replay()
                        g.replay()
                        sched.step()
                torch.cuda.synchronize()
                assert not ops.TwoStream.active
                finals[two, mode] = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu()
                losses[two, mode] = float(loss)
    finally:
        ops.set_two_stream(True)          # the default
        ops.set_matmul_precision("fp32")
        ops.DropoutState.manual_seed(None)
    ref = finals[False, "eager"]
    assert torch.isfinite(ref).all()
    for key, val in finals.items():
        assert losses[key] == losses[False, "eager"], (key, losses)
        assert torch.equal(val, ref), (key, float((val - ref).abs().max()))
    # dropout really was on: the same run in eval-like p = 0 lands elsewhere
    ops.DropoutState.manual_seed(1234)
    try:
        model, _ = build_lily(dev, cfg, args, seed=11, **SWISH)
        model.train()
        opt, sched, _, _ = get_optimization(args, model, 10, None)
        ops.set_matmul_precision(precision)
        for i in range(5):
            U.train_step(model, opt, sched, batch, args, i, all_options=True)
    finally:
        ops.set_matmul_precision("fp32")
        ops.DropoutState.manual_seed(None)
    assert not torch.equal(torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu(), ref)


def test_swish_config_json_trains_saves_resumes_and_evaluates(dev, lib, tmp_path):
    """A BertConfig JSON with "hidden_act": "swish" through train_epoch, save_model, get_optimization(--resume) and the evaluation loops
    (the test_save_resume_and_eval_loops pattern): the resumed run continues like the uninterrupted one."""
    from ytvln import synth
    from ytvln import utils_init as U
    from ytvln.lily import Lily
    from ytvln.vilbert import BertConfig
    from ytvln.vilbert_init import get_optimization
    path = tmp_path / "swish.json"
    json.dump(cfg_dict("micro.json", **ZERO_DROP, **SWISH), open(path, "w"))
    args = args_ns(ranking=True, masked_vision=True, masked_language=True)      # (no trajectory head: NaN on a ragged opt_mask, see g0)
    args.learning_rate = 1e-3
    loader = [synth.to_torch(synth.make_batch(bs=3, K=7, T=8, frames=2, boxes=3, F=16, C=11, vocab=97, seed=90 + i, opt_holes=(i % 2),
                                             ignore_rank_frac=0.0)) for i in range(4)]

    def fresh():
        cfg = BertConfig.from_json_file(str(path))
        assert cfg.hidden_act == "swish" and cfg.v_hidden_act == "swish"
        cfg.args = args
        m = Lily(cfg, dropout_prob=0.0)
        W = synth.make_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, 17)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
        return m.to(dev).train()

    m0 = fresh()
    o0, s0, _, _ = get_optimization(args, m0, 10, None)
    before = torch.cat([p.detach().reshape(-1) for p in m0.parameters()]).clone()
    U.train_epoch(0, m0, o0, s0, loader, None, True, args, None)
    U.train_epoch(1, m0, o0, s0, loader, None, True, args, None)
    a = torch.cat([p.detach().reshape(-1) for p in m0.parameters()])
    assert bool(torch.isfinite(a).all()) and float((a - before).abs().max()) > 0
    # one epoch, saved, resumed into a fresh model, second epoch
    m1 = fresh()
    o1, s1, _, _ = get_optimization(args, m1, 10, None)
    U.train_epoch(0, m1, o1, s1, loader, None, True, args, None)
    U.save_model(str(tmp_path), "ckpt", None, m1, o1, s1, epoch=0)
    m2 = fresh()
    rargs = args_ns(**{**vars(args), "resume": True, "from_pretrained": U.get_model_path(str(tmp_path), "ckpt")})
    o2, s2, _, start_epoch = get_optimization(rargs, m2, 10, None)
    assert start_epoch == 1
    U.train_epoch(1, m2, o2, s2, loader, None, True, args, None)
    b = torch.cat([p.detach().reshape(-1) for p in m2.parameters()])
    assert float((a - b).abs().max()) < 2e-6, float((a - b).abs().max())
    # evaluation loops against a direct evaluation
    nb = synth.make_batch(bs=2, K=3, T=8, frames=2, boxes=3, F=16, C=11, vocab=97, seed=21, ignore_rank_frac=0.0)
    tgt = np.zeros((2, 3), bool); tgt[0, 0] = True; tgt[1, 1] = True
    eb = list(nb); eb[0] = tgt
    ev = [synth.to_torch(eb), synth.to_torch(eb)]
    sr = U.val_epoch(0, m0, "val_seen", ev, None, True, args, 0, None, "ranking")
    red = U.test_epoch(0, m0, "test", ev, None, True, args, 0, None)
    assert set(red) == {"ranking"}
    m0.eval()
    with torch.no_grad():
        out = m0(*U.get_model_input(synth.to_torch(eb, dev), True))
    logit = out["ranking"].view(2, 3).double()
    t = torch.from_numpy(tgt).to(dev)
    ref_loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, t.double())
    ref_sr = t.gather(1, logit.argmax(1, keepdim=True)).double().sum() / 2
    assert abs(float(sr) - float(ref_sr)) < 1e-6
    assert abs(float(red["ranking"][1]) - float(ref_loss)) < 1e-5 and abs(float(red["ranking"][2]) - float(ref_sr)) < 1e-6


# ------------------------------------------------------------------------------------------------------------------
# 8: the design -- gelu configurations never reach the activation kernel
# ------------------------------------------------------------------------------------------------------------------
def test_gelu_configs_never_call_act_fwd(dev, lib, monkeypatch):
    from ytvln import _lib, ops, synth
    from ytvln import utils_init as U
    from ytvln.vilbert_init import get_optimization
    counts = {}
    real = _lib.call

    def counting(name, *a):
        counts[name] = counts.get(name, 0) + 1
        return real(name, *a)

    monkeypatch.setattr(_lib, "call", counting)
    monkeypatch.setattr(ops, "call", counting)          # (ops binds the name at import)
    args = args_ns(**ALL)
    args.learning_rate = 1e-3
    batch = synth.to_torch(synth.make_batch(bs=2, K=3, T=8, frames=2, boxes=3, F=16, C=11, vocab=97, seed=21, ignore_rank_frac=0.0), dev)
    seen = {}
    for name, acts in (("gelu", {}), ("relu", dict(hidden_act="relu", v_hidden_act="relu")), ("swish", SWISH)):
        for precision in ("fp32", "bf16"):
            counts.clear()
            model, _ = build_lily(dev, "tiny_2_2_1.json" if precision == "bf16" else "micro.json", args, seed=11, **acts)
            model.train()
            opt, sched, _, _ = get_optimization(args, model, 10, None)
            b = batch if precision == "fp32" else synth.to_torch(synth.make_batch(bs=2, K=7, T=16, frames=2, boxes=4, seed=22, ignore_rank_frac=0.0), dev)
            ops.set_matmul_precision(precision)
            try:
                U.train_step(model, opt, sched, b, args, 0, all_options=True)
                model.eval()
                with torch.no_grad():
                    model(*U.get_model_input(b, True))
            finally:
                ops.set_matmul_precision("fp32")
            torch.cuda.synchronize()
            seen[name, precision] = sum(v for k, v in counts.items() if k.startswith("ytvln_act_fwd"))
            assert any(k.startswith("ytvln_gemm") for k in counts), "the wrapper saw no GEMM call: it is not in the call path"
    print(f"[act_fwd calls per train step + eval forward] {seen}")
    assert all(seen[a, p] == 0 for a in ("gelu", "relu") for p in ("fp32", "bf16")), seen
    assert all(seen["swish", p] > 0 for p in ("fp32", "bf16")), seen
