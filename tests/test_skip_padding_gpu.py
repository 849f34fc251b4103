"""GPU: padding-free execution (BertModel.skip_padding) -- the row plan against torch.nonzero, the row mover bit for bit against torch
indexing, the adjoint property, and the model with both streams on packed rows against oracle/vilbert_ref.py run on the CPU.

Bars: fp32 |loss - ref| <= 1e-4, outputs 1e-4 + 1e-4 |ref|, per-tensor gradient rel-L2 <= 1e-4 (tensors whose reference
norm is below 1e-7 -- key biases, mathematically zero -- are exempt, as everywhere in the suite); bf16-resident path: losses and outputs within
2e-2 relative, gradient norms within 5 % (+1e-4).  Dropout is off wherever values are compared with a reference; with dropout on only
bit-reproducibility is asserted (the LayerNorm / FFN sites of a packed run hash packed coordinates)."""
import functools

import numpy as np
import pytest
import torch

from helpers import ZERO_DROP, args_ns, cfg_dict, close, rel_l2

pytestmark = pytest.mark.gpu

LOSS_TOL = 1e-4


# ---------------------------------------------------------------------------------------------------------------------------------------
# plan
# ---------------------------------------------------------------------------------------------------------------------------------------
def _flags(kind, rows, seed):
    if kind == "zeros":
        return torch.zeros(rows, dtype=torch.int64)
    if kind == "ones":
        return torch.ones(rows, dtype=torch.int64)
    if kind == "last":
        f = torch.zeros(rows, dtype=torch.int64)
        f[-1] = 1
        return f
    return (torch.rand(rows, generator=torch.Generator().manual_seed(seed)) < 0.5).to(torch.int64)


@pytest.mark.parametrize("rows", [1, 65, 1025, 40000])
def test_plan_equals_nonzero(dev, lib, rows):
    from ytvln import ops
    for kind in ("zeros", "ones", "random", "last"):
        flags = _flags(kind, rows, rows)
        where = torch.nonzero(flags).reshape(-1)
        count = int(where.numel())
        for cap in sorted({1, count - 1, count, count + 300, rows}):
            if cap < 1:
                continue
            for f in (flags, flags.to(torch.float32) * 2.5, flags.bool()):          # non-zero = valid, whatever the mask's dtype
                plan = ops.rows_plan(f.to(dev), cap)
                assert (plan.rows, plan.capacity) == (rows, cap)
                fit = where[:cap]
                pack = torch.full((cap,), -1, dtype=torch.int64)
                pack[:fit.numel()] = fit
                unpack = torch.full((rows,), -1, dtype=torch.int64)
                unpack[fit] = torch.arange(fit.numel())
                assert torch.equal(plan.pack_idx.cpu(), pack), (kind, rows, cap)
                assert torch.equal(plan.unpack_idx.cpu(), unpack), (kind, rows, cap)
                assert plan.counts.tolist() == [count, max(count - cap, 0)], (kind, rows, cap, plan.counts.tolist())


# ---------------------------------------------------------------------------------------------------------------------------------------
# mover
# ---------------------------------------------------------------------------------------------------------------------------------------
def _move_raw(x, ld, x_rows, idx, out, ldo, width):
    from ytvln import _lib, ops
    _lib.call("ytvln_rows_move_bf16" if x.dtype == torch.bfloat16 else "ytvln_rows_move_f32", x.data_ptr(), ld, x_rows, idx.data_ptr(), idx.numel(), width,
              out.data_ptr(), ldo, ops._stream())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_mover_is_torch_indexing_bit_for_bit(dev, lib, dtype):
    g = torch.Generator().manual_seed(3)
    x_rows = 37
    idx = torch.randint(0, x_rows, (50,), generator=g)
    idx[::7] = -1
    idx[3] = x_rows + 5          # out of range: a zero row, never a read
    idx = idx.to(dev)
    live = ((idx >= 0) & (idx < x_rows)).unsqueeze(1)
    safe = idx.clamp(0, x_rows - 1)
    # (width, leading dimension of x, of out, column offset into x, element offset of both base pointers)
    cases = [(w, w, w, 0, 0) for w in (1, 3, 4, 12, 768, 2048)]
    cases += [(w, w + 5, w + 3, 0, 0) for w in (1, 3, 4, 12, 768)]            # ld > width, no 16-byte alignment of the rows
    cases += [(w, w + 8, w + 16, 0, 0) for w in (4, 12, 768, 2048)]            # ld > width, aligned: the 16-byte path with untouched columns behind
    cases += [(768, 2304, 768, 768, 0), (768, 2304, 776, 1536, 0)]             # the k window of a q|k|v matrix
    cases += [(w, w + 8, w + 8, 0, 1) for w in (3, 12, 768)]                   # base pointers off by one element
    cases += [(13, 24, 16, 0, 0), (771, 776, 776, 0, 0)]                       # 16-byte vectors plus an element tail
    for width, ldx, ldo, col, off in cases:
        xbuf = torch.randn(x_rows * ldx + 8, generator=g).to(dtype).to(dev)
        x = xbuf[off:off + x_rows * ldx].view(x_rows, ldx)
        want_rows = torch.where(live, x[safe, col:col + width], torch.zeros((), dtype=dtype, device=dev))
        for n_out in (50, 1, 0):
            obuf = torch.full((50 * ldo + 8,), 7.0, dtype=dtype, device=dev)          # sentinel
            out = obuf[off:off + 50 * ldo].view(50, ldo)
            _move_raw(x[:, col:], ldx, x_rows, idx[:n_out], out, ldo, width)
            torch.cuda.synchronize()
            want = torch.full_like(obuf, 7.0)
            want[off:off + 50 * ldo].view(50, ldo)[:n_out, :width] = want_rows[:n_out]
            assert torch.equal(obuf.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                               want.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)), (width, ldx, ldo, col, off, n_out)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pack_unpack_values_and_adjoint(dev, lib, dtype):
    """rows_pack / rows_unpack and their gradients equal torch's indexing and its gradients exactly (each output element has one source, so
    there is no sum whose order could differ)."""
    from ytvln import ops
    g = torch.Generator().manual_seed(5)
    rows, W = 300, 40
    mask = (torch.rand(rows, generator=g) < 0.5)
    mask[0] = True
    for cap in (int(mask.sum()) + 20, int(mask.sum()) - 9):          # room to spare / overflow
        plan = ops.rows_plan(mask.to(dev), cap)
        where = torch.nonzero(mask).reshape(-1)[:cap].to(dev)
        # pack (from a strided column window: read through pointer + leading dimension)
        base = torch.randn(rows, 3 * W, generator=g).to(dtype).to(dev)
        for window in (lambda b: b[:, W:2 * W], lambda b: b[:, :W].reshape(10, 30, W)):          # in place through (pointer, ld) / any leading shape
            ba, bb = base.clone().requires_grad_(True), base.clone().requires_grad_(True)
            ya = ops.rows_pack(window(ba), plan)
            yb = torch.zeros(cap, W, dtype=dtype, device=dev).index_put((torch.arange(where.numel(), device=dev),), window(bb).reshape(rows, W)[where])
            assert ya.shape == (cap, W) and torch.equal(ya, yb)
            cot = torch.randn(cap, W, generator=g).to(dtype).to(dev)
            ya.backward(cot)
            yb.backward(cot)
            assert torch.equal(ba.grad, bb.grad) and bool(ba.grad.any())
        # unpack
        pa = torch.randn(cap, W, generator=g).to(dtype).to(dev).requires_grad_(True)
        pb = pa.detach().clone().requires_grad_(True)
        ua = ops.rows_unpack(pa, plan)
        ub = torch.zeros(rows, W, dtype=dtype, device=dev).index_put((where,), pb[:where.numel()])
        assert ua.shape == (rows, W) and torch.equal(ua, ub)
        cot = torch.randn(rows, W, generator=g).to(dtype).to(dev)
        ua.backward(cot)
        ub.backward(cot)
        assert torch.equal(pa.grad, pb.grad)
        assert torch.equal(pa.grad[where.numel():], torch.zeros_like(pa.grad[where.numel():]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# model
# ---------------------------------------------------------------------------------------------------------------------------------------
FLAGS = dict(ranking=True, traj_judge=True, masked_vision=True, masked_language=True)
SHAPES = {"micro.json": dict(bs=4, K=7, T=16, frames=2, boxes=6, F=16, C=11, vocab=97, seed=41, ignore_rank_frac=0.0),
          "tiny_2_2_1.json": dict(bs=4, K=7, T=16, frames=2, boxes=6, seed=42, ignore_rank_frac=0.0)}
# 28 pairs: 448 text rows and 336 image rows, about half of them valid -> "exact" and 0.5 both give one 256-row tile per side


def crafted_batch(cfgname, empty_pair=False, full=False, seed=7):
    """synth.make_batch is full at these sizes: the masks are crafted here.  Valid fraction about 0.5, valid and padded rows interleaved, row 0 of
    every pair valid (the poolers read it), pair 0 with a single valid token and a single valid region; targets only on valid rows (no loss
    reads a padded row, as in the real data).  `empty_pair`: pair 1 has no valid region at all (finiteness only).  `full`: every row valid."""
    from ytvln import synth
    nb = synth.make_batch(**SHAPES[cfgname])
    rs = np.random.RandomState(seed)
    tmask = rs.rand(*nb[7].shape) < (2.0 if full else 0.5)
    vmask = rs.rand(*nb[3].shape) < (2.0 if full else 0.5)
    tmask[..., 0] = True
    vmask[..., 0] = True
    if not full:
        tmask[0, 0, 1:] = False
        vmask[0, 0, 1:] = False
    if empty_pair:
        vmask[0, 1, :] = False
    nb[7] = tmask
    nb[3] = vmask.astype(np.int64)
    nb[6] = np.where(tmask, nb[6], 0)
    nb[8] = np.where(tmask, nb[8], -1)
    nb[5] = np.where(vmask, nb[5], 0)
    assert (nb[8] != -1).sum() > 10 and nb[5].sum() > 10
    return nb


def build_lily(dev, cfgname, seed=11, dropout=0.0, **over):
    from ytvln import synth
    from ytvln.lily import Lily
    from ytvln.vilbert import BertConfig
    args = args_ns(**FLAGS)
    cfg = BertConfig(**cfg_dict(cfgname, **{**ZERO_DROP, **over}))
    cfg.args = args
    model = Lily(cfg, dropout_prob=dropout)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    W = synth.make_weights(shapes, seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    return model.to(dev).train(), W, args


def run(model, batch, args, backward=True):
    """-> (per-task losses, total, (seq_t, seq_v), {name: grad or None})."""
    from ytvln import utils_init as U
    seen = {}
    hook = model.bert.register_forward_hook(lambda m, i, o: seen.__setitem__("seq", (o[0].detach(), o[1].detach())))
    try:
        for p in model.parameters():
            p.grad = None
        outputs = model(*U.get_model_input(batch, all_options=True))
    finally:
        hook.remove()
    per, total = {}, None
    for task, flag in U.TASKS:
        _, _, l, _ = U.get_loss_correct(batch, outputs, task, args, None, True, all_options=True)
        per[task] = l
        l = args.traj_loss_scale * l if task == "traj" else l
        total = l if total is None else total + l
    if backward:
        total.backward()
        ops_join()
    grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}
    return {k: float(v.detach()) for k, v in per.items()}, float(total.detach()), seen["seq"], grads


def ops_join():
    from ytvln import ops
    ops.TwoStream.join_backward()
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def oracle(cfgname):
    """The reference's losses, sequence outputs and gradients for crafted_batch(cfgname) with build_lily's weights: computed once, on the CPU."""
    import vilbert_ref as O
    from ytvln import synth
    from ytvln.lily import Lily
    from ytvln.vilbert import BertConfig
    cfg = BertConfig(**cfg_dict(cfgname, **ZERO_DROP))
    cfg.args = args_ns(**FLAGS)
    shapes = {k: tuple(v.shape) for k, v in Lily(cfg, dropout_prob=0.0).state_dict().items()}
    W = O.trainable({k: torch.from_numpy(v).clone() for k, v in synth.make_weights(shapes, 11).items()})
    cb = synth.to_torch(crafted_batch(cfgname))
    flags = O.TaskFlags(**FLAGS)
    collect = {}
    out = O.lily_forward(W, O.RefConfig(**cfg_dict(cfgname, **ZERO_DROP)), flags, *O.model_input(cb), collect=collect)
    total, per = O.total_loss(cb, out, flags)
    total.backward()
    grads = {k: (None if v.grad is None else v.grad.detach()) for k, v in W.items() if k != "cls.predictions.decoder.weight"}
    return ({k: float(v.detach()) for k, v in per.items()}, float(total.detach()), collect["sequence_output_t"].detach(), collect["sequence_output_v"].detach(), grads)


def valid_masks(nb, dev):
    return torch.from_numpy(nb[7]).flatten(0, 1).to(dev), torch.from_numpy(nb[3] > 0).flatten(0, 1).to(dev)


@pytest.mark.parametrize("precision,cfgname,mode", [("fp32", "micro.json", "exact"), ("fp32", "micro.json", (0.5, 0.5)),
                                                    ("bf16", "tiny_2_2_1.json", "exact")])
def test_packed_model_against_the_cpu_oracle(dev, lib, precision, cfgname, mode):
    from ytvln import ops, synth
    nb = crafted_batch(cfgname)
    batch = synth.to_torch(nb, dev)
    mt, mv = valid_masks(nb, dev)
    oper, ototal, oseq_t, oseq_v, ograds = oracle(cfgname)
    model, _, args = build_lily(dev, cfgname)
    ops.set_matmul_precision(precision)
    try:
        assert model.bert.skip_padding is None
        pper, ptotal, _, _ = run(model, batch, args)                              # the padded run of the same build
        model.bert.skip_padding = mode
        per, total, (seq_t, seq_v), grads = run(model, batch, args)
    finally:
        ops.set_matmul_precision("fp32")
    assert model.bert.padding_overflow.tolist() == [0, 0]
    print(f"[skip_padding {precision} {mode}] oracle {oper} padded {pper} packed {per}")
    # returned padded rows are exact zeros, valid rows are not
    assert seq_t.shape == oseq_t.shape and seq_v.shape == oseq_v.shape
    assert not bool(seq_t[~mt].any()) and not bool(seq_v[~mv].any())
    assert bool(seq_t[mt].float().abs().sum(-1).min() > 0) and bool(seq_v[mv].float().abs().sum(-1).min() > 0)
    none_ref = {n for n, g in ograds.items() if g is None}
    assert {n for n, g in grads.items() if g is None} == none_ref
    if precision == "fp32":
        for k in oper:
            assert abs(per[k] - oper[k]) <= LOSS_TOL, (k, per[k], oper[k])
            assert abs(per[k] - pper[k]) <= LOSS_TOL, (k, per[k], pper[k])
        assert abs(total - ototal) <= LOSS_TOL
        close(seq_t[mt], oseq_t[mt.cpu()], 1e-4, 1e-4, "sequence_output_t (valid rows)")
        close(seq_v[mv], oseq_v[mv.cpu()], 1e-4, 1e-4, "sequence_output_v (valid rows)")
        bad = {n: rel_l2(g, ograds[n]) for n, g in grads.items() if g is not None
               and not (rel_l2(g, ograds[n]) <= 1e-4 or float(ograds[n].norm()) < 1e-7)}
        assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]
    else:
        for k in oper:
            assert abs(per[k] - oper[k]) <= 2e-2 * max(abs(oper[k]), 1e-3), (k, per[k], oper[k])
            assert abs(per[k] - pper[k]) <= LOSS_TOL, (k, per[k], pper[k])
        assert rel_l2(seq_t[mt].float(), oseq_t[mt.cpu()]) <= 2e-2 and rel_l2(seq_v[mv].float(), oseq_v[mv.cpu()]) <= 2e-2
        bad = [(n, float(g.double().norm()), float(ograds[n].norm())) for n, g in grads.items() if g is not None
               and abs(float(g.double().norm()) - float(ograds[n].norm())) > 5e-2 * float(ograds[n].norm()) + 1e-4]
        assert not bad, bad[:8]


def test_pair_without_a_valid_region_stays_finite(dev, lib):
    from ytvln import synth
    batch = synth.to_torch(crafted_batch("micro.json", empty_pair=True), dev)
    model, _, args = build_lily(dev, "micro.json")
    model.bert.skip_padding = "exact"
    per, total, (seq_t, seq_v), grads = run(model, batch, args)
    assert np.isfinite(total) and all(np.isfinite(v) for v in per.values())
    assert bool(torch.isfinite(seq_t).all()) and bool(torch.isfinite(seq_v).all())
    assert all(bool(torch.isfinite(g).all()) for g in grads.values() if g is not None)


def test_two_stream_equals_one_stream_on_packed_rows(dev, lib):
    from ytvln import ops, synth
    batch = synth.to_torch(crafted_batch("micro.json"), dev)
    got = []
    was = ops.get_two_stream()
    try:
        for flag in (True, False):
            ops.set_two_stream(flag)
            model, _, args = build_lily(dev, "micro.json")
            model.bert.skip_padding = (0.5, 0.5)
            got.append(run(model, batch, args))
    finally:
        ops.set_two_stream(was)
    (pa, ta, sa, ga), (pb, tb, sb, gb) = got
    assert pa == pb and ta == tb and torch.equal(sa[0], sb[0]) and torch.equal(sa[1], sb[1])
    for n in ga:
        assert (ga[n] is None) == (gb[n] is None) and (ga[n] is None or torch.equal(ga[n], gb[n])), n


DROP = dict(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, v_attention_probs_dropout_prob=0.1, v_hidden_dropout_prob=0.1)


def test_dropout_on_is_reproducible_and_recompute_tiers_are_bit_identical(dev, lib):
    from ytvln import ops, synth
    batch = synth.to_torch(crafted_batch("micro.json"), dev)
    got = {}
    try:
        for name, tier in (("none", "none"), ("again", "none"), ("layer", "layer"), ("ffn", "ffn")):
            model, _, args = build_lily(dev, "micro.json", dropout=0.1, **DROP)
            model.bert.skip_padding = 0.5
            model.bert.encoder.recompute = tier
            ops.DropoutState.manual_seed(1234)
            got[name] = run(model, batch, args)
    finally:
        ops.DropoutState.manual_seed(None)
    per0, total0, seq0, g0 = got["none"]
    zero_drop_model, _, args = build_lily(dev, "micro.json")
    zero_drop_model.bert.skip_padding = 0.5
    assert run(zero_drop_model, batch, args)[1] != total0, "dropout did not run"
    for name in ("again", "layer", "ffn"):
        per, total, seq, g = got[name]
        assert per == per0 and total == total0, (name, per, per0)
        assert torch.equal(seq[0], seq0[0]) and torch.equal(seq[1], seq0[1]), name
        for n in g0:
            assert (g[n] is None) == (g0[n] is None) and (g[n] is None or torch.equal(g[n], g0[n])), (name, n)


def test_encoder_cut_points_on_packed_rows(dev, lib):
    """encoder.cut_after (the phased backward of GraphedTrainStep) cuts packed hidden states like padded ones: a backward run phase by phase
    through the recorded cuts launches the same kernels on the same inputs as the one-pass backward -- the same bits."""
    from ytvln import synth
    batch = synth.to_torch(crafted_batch("micro.json"), dev)
    model, _, args = build_lily(dev, "micro.json")
    model.bert.skip_padding = 0.5
    _, total0, _, g0 = run(model, batch, args)
    model.bert.encoder.cut_after = frozenset({"t0", "v0", "c0"})
    try:
        _, total1, _, _ = run(model, batch, args)          # backward down to the leaves above the top-most cut
        cuts = model.bert.encoder._cuts
        assert [c[0] for c in cuts] == ["v0", "t0", "c0"] and all(h.shape[0] == 1 for c in cuts for h in c[1])          # packed [1, capacity, H]
        for _, below, above in reversed(cuts):
            torch.autograd.backward(below, [a.grad for a in above])
        ops_join()
    finally:
        model.bert.encoder.cut_after = frozenset()
    assert total1 == total0
    for n, p in model.named_parameters():
        assert (p.grad is None) == (g0[n] is None) and (p.grad is None or torch.equal(p.grad, g0[n])), n


def test_capacity_too_small_is_counted_and_stays_finite(dev, lib):
    from ytvln import synth
    from ytvln import utils_init as U
    from ytvln.vilbert_init import get_optimization
    batch = synth.to_torch(crafted_batch("micro.json", full=True), dev)          # 448 / 336 valid rows against one 256-row tile per side
    model, _, args = build_lily(dev, "micro.json")
    model.bert.skip_padding = (0.5, 0.4)
    per, total, (seq_t, seq_v), grads = run(model, batch, args)
    assert model.bert.padding_overflow.tolist() == [448 - 256, 336 - 256]
    assert np.isfinite(total) and bool(torch.isfinite(seq_t).all()) and bool(torch.isfinite(seq_v).all())
    assert all(bool(torch.isfinite(g).all()) for g in grads.values() if g is not None)
    args.learning_rate = 1e-3
    opt, sched, _, _ = get_optimization(args, model, 10, None)
    loss, metrics = U.train_step(model, opt, sched, batch, args, 0, all_options=True)
    assert metrics["padding_row_overflow"].numel() == 1 and float(metrics["padding_row_overflow"]) == 2 * (192 + 80)
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p).all()) for p in model.parameters())
    model.bert.skip_padding = None
    assert "padding_row_overflow" not in U.train_step(model, opt, sched, batch, args, 1, all_options=True)[1]


def test_exact_raises_under_capture_and_static_capacity_replays(dev, lib):
    """A hipGraph of forward + backward with a static capacity, replayed after tokens, features, masks and targets were refilled in place,
    equals the eager run on the new batch bit for bit (the bar of tests/test_model_gpu.py::test_graph_replay_equals_eager)."""
    from ytvln import synth
    from ytvln import utils_init as U
    first, second = crafted_batch("micro.json", seed=7), crafted_batch("micro.json", seed=8)
    second[6] = np.where(second[7], np.roll(second[6], 3, axis=-1), 0)          # other tokens, other features, other masks
    second[6][..., 0] = first[6][..., 0]
    second[1] = second[1][::-1].copy()
    static = synth.to_torch(first, dev)
    model, _, args = build_lily(dev, "micro.json")
    model.bert.skip_padding = (0.6, 0.6)

    def step():
        for p in model.parameters():
            p.grad = None
        return U.train_step(model, None, None, static, args, 0, all_options=True, optimizer_step=False)[0]

    for _ in range(2):
        step()
    torch.cuda.synchronize()
    model.bert.skip_padding = "exact"
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="exact"):
        with torch.cuda.graph(g):
            step()
    torch.cuda.synchronize()
    model.bert.skip_padding = (0.6, 0.6)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss = step()
    for dst, src in zip(static, synth.to_torch(second, dev)):
        dst.copy_(src)
    g.replay()
    torch.cuda.synchronize()
    replayed = float(loss), {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}
    eager = float(step())
    ops_join()
    assert replayed[0] == eager, (replayed[0], eager)
    for n, p in model.named_parameters():
        assert (p.grad is None) == (replayed[1][n] is None) and (p.grad is None or torch.equal(p.grad, replayed[1][n])), n
    assert model.bert.padding_overflow.tolist() == [0, 0]


def test_vltasks_forward_backward_on_packed_rows(dev, lib):
    """VILBertForVLTasks: the seven outputs on valid rows and every gradient of a loss that reads valid rows only, against the fp32 restatement
    of the model on the CPU (tests/vltasks_common.py)."""
    import vilbert_ref as O
    import vltasks_common as C
    from ytvln import synth
    nb = synth.make_batch(bs=30, K=1, T=12, frames=2, boxes=5, F=16, C=11, vocab=97, seed=31)          # 360 text rows, 300 image rows
    rs = np.random.RandomState(9)
    tmask, vmask = rs.rand(30, 1, 12) < 0.5, rs.rand(30, 10) < 0.5
    tmask[..., 0], vmask[..., 0] = True, True
    tmask[0, 0, 1:], vmask[0, 1:] = False, False
    nb[7] = tmask
    model = C.build_model("micro.json")
    W = C.make_weights(model, 13)
    model.load_state_dict(C.state_of(W))
    model.to(dev).train()
    model.bert.skip_padding = "exact"
    row_masks = {3: vmask, 4: vmask, 5: tmask[:, 0], 6: tmask[:, 0]}          # the per-row outputs (C.OUT_NAMES) and the rows that count

    def loss_of(outs):
        cs = C.cotangents([o.shape for o in outs], 17)
        total = 0.0
        for i, (o, c) in enumerate(zip(outs, cs)):
            c = torch.from_numpy(c).to(o.device).double()
            if i in row_masks:
                m = torch.from_numpy(row_masks[i]).to(o.device).unsqueeze(-1)
                total = total + (torch.where(m, o.double(), torch.zeros((), dtype=torch.float64, device=o.device)) * c).sum()
            else:
                total = total + (o.double() * c).sum()
        return total

    outs = model(*C.inputs_of(nb, vmask.astype(np.int64), dev))
    loss = loss_of(outs)
    loss.backward()
    ops_join()
    S = O.trainable(C.state_of(W))
    routs = C.vltasks_forward(S, O.RefConfig(**cfg_dict("micro.json", **ZERO_DROP)), *C.inputs_of(nb, vmask.astype(np.int64)))
    rloss = loss_of(routs)
    rloss.backward()
    assert abs(float(loss.detach()) - float(rloss.detach())) <= LOSS_TOL, (float(loss.detach()), float(rloss.detach()))
    for i, (o, r) in enumerate(zip(outs, routs)):
        if i in row_masks:
            m = torch.from_numpy(row_masks[i])
            close(o.detach().cpu()[m], r.detach()[m], 1e-4, 1e-4, C.OUT_NAMES[i])
        else:
            close(o, r, 1e-4, 1e-4, C.OUT_NAMES[i])
    assert model.bert.padding_overflow.tolist() == [0, 0]
    ref = {k: v.grad for k, v in S.items() if k != "cls.predictions.decoder.weight"}
    assert {n for n, p in model.named_parameters() if p.grad is None} == {n for n, g in ref.items() if g is None}
    bad = {n: rel_l2(p.grad, ref[n]) for n, p in model.named_parameters() if p.grad is not None
           and not (rel_l2(p.grad, ref[n]) <= 1e-4 or float(ref[n].norm()) < 1e-7)}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]


def test_default_is_off_and_launches_nothing_new(dev, lib, monkeypatch):
    from ytvln import _lib, ops, synth
    from ytvln.vilbert import BertModel
    assert BertModel.skip_padding is None
    batch = synth.to_torch(crafted_batch("micro.json"), dev)
    model, _, args = build_lily(dev, "micro.json")
    assert model.bert.skip_padding is None
    names = []
    real = _lib.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)

    monkeypatch.setattr(_lib, "call", spy)
    monkeypatch.setattr(ops, "call", spy)          # (ops binds the function by name at import)
    run(model, batch, args)
    assert names and not [n for n in names if n.startswith("ytvln_rows_")], sorted(set(names))
    assert model.bert.padding_overflow is None
    del names[:]
    model.bert.skip_padding = 0.5
    run(model, batch, args)
    assert {"ytvln_rows_plan", "ytvln_rows_move_f32"} <= set(names)
    for bad in (0.0, "yes", (0.5, 0.5, 0.5)):
        model.bert.skip_padding = bad
        with pytest.raises(ValueError, match="BertModel.skip_padding"):
            run(model, batch, args)


def test_in_batch_pairs_and_fast_mode_are_refused(dev, lib):
    from ytvln import synth
    batch = synth.to_torch(crafted_batch("micro.json"), dev)
    for over in (dict(in_batch_pairs=True), dict(fast_mode=True)):
        model, _, args = build_lily(dev, "micro.json", **over)
        model.bert.skip_padding = 0.5
        with pytest.raises(NotImplementedError, match="skip_padding"):
            run(model, batch, args)
