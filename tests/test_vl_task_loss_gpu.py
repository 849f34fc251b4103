"""Row-wise BCE kernels (csrc/task_loss.hip), ops.bce_with_logits_rows and ytvln/vl_tasks.py on the GPU against the fp64 restatements of
tests/vl_task_ref.py.

Kernel bars are those of tests/test_kernels_gpu.py for the loss kernels ("kl big", "bce"): loss within 2e-6 + 2e-6 |ref|, gradient rel-L2
< 1e-6; row_top equals torch.argmax, the score is the fp64 sum of the gathered targets to 1e-6 relative.  Model bars are the fp32 bars of
DESIGN.md section 2: |dL| <= 1e-4, every gradient at rel-L2 <= 1e-4 (only the tensors whose gradient is identically
zero are excluded, by name, and held to an absolute size: _identically_zero),
parameter norms after three AdamW steps within 2e-6 relative.  Each figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

from helpers import ZERO_DROP, args_ns, cfg_dict, close, gold, rel_l2
from vl_task_ref import bce_rows_ref, kernel_inputs, task_loss_ref
from vltasks_common import MICRO_BATCH, NUM_LABELS, build_model, inputs_of, make_weights, state_of, vltasks_forward

pytestmark = pytest.mark.gpu

SHAPES = [(3, 1, None), (5, 57, None), (7, 256, None), (4, 3129, 3136), (33, 3129, None), (300, 259, None)]
_INPUTS = {}


def _inputs(M, C, huge=True):
    """CPU fp32 (x, t) of one shape, made once and never modified."""
    key = (M, C, huge)
    if key not in _INPUTS:
        _INPUTS[key] = kernel_inputs(M, C, seed=1000 + 7 * M + C, huge=huge)
    return _INPUTS[key]


def _pos_weight(kind, C):
    if kind == "none":
        return None
    if kind == "scalar":
        return torch.tensor([2.5])
    return torch.from_numpy((0.5 + 2.0 * np.random.RandomState(C).random_sample(C)).astype(np.float32))


def _on_device(x, dev, ld=None):
    """A device copy of x; with ld the rows sit in a [M, ld] buffer (NaN in the padding: reading it would poison the loss)."""
    if ld is None:
        return x.to(dev)
    full = torch.full((x.shape[0], ld), float("nan"), device=dev)
    full[:, :x.shape[1]] = x.to(dev)
    return full[:, :x.shape[1]]


def _check_against_fp64(dev, M, C, ld, kind, huge=True):
    from ytvln import ops
    x, t = _inputs(M, C, huge)
    pw = _pos_weight(kind, C)
    xd = x.double().requires_grad_(True)
    ref, ref_score, ref_top = bce_rows_ref(xd, t, pw, scale=float(C))
    ref.backward()
    xg = _on_device(x, dev, ld).requires_grad_(True)
    assert ld is None or (xg.stride(0) == ld and not xg.is_contiguous())
    tg = _on_device(t, dev, None if ld is None else ld + 24)          # the targets through a leading dimension of their own
    loss, score, top = ops.bce_with_logits_rows(xg, tg, None if pw is None else pw.to(dev), scale=float(C))
    assert loss.shape == () and loss.dtype == torch.float32 and loss.requires_grad
    assert score.shape == () and not score.requires_grad and top.shape == (M,) and top.dtype == torch.int64 and not top.requires_grad
    loss.backward()
    torch.cuda.synchronize()
    err, rg = abs(float(loss) - float(ref)), rel_l2(xg.grad, xd.grad)
    print(f"[bce rows {M}x{C} ld={ld} pw={kind} huge={huge}] loss {float(loss):.9g} vs {float(ref):.9g} (|d| {err:.2e}, rel {err / abs(float(ref)):.2e}), "
          f"gradient rel-L2 {rg:.2e}, score {float(score):.7g} vs {float(ref_score):.7g}")
    close(loss, ref.detach(), 2e-6, 2e-6, "loss")
    assert xg.grad.shape == (M, C) and rg < 1e-6, rg
    assert torch.equal(top.cpu(), ref_top) and torch.equal(ref_top, torch.argmax(x, 1))
    assert abs(float(score) - float(ref_score)) <= 1e-6 * max(abs(float(ref_score)), 1e-30) or float(score) == float(ref_score)


@pytest.mark.parametrize("kind", ["none", "scalar", "per_class"])
@pytest.mark.parametrize("M,C,ld", SHAPES)
def test_kernel_against_the_fp64_restatement(dev, lib, M, C, ld, kind):
    _check_against_fp64(dev, M, C, ld, kind)


def test_kernel_against_the_fp64_restatement_without_the_huge_logits(dev, lib):
    _check_against_fp64(dev, 33, 3129, None, "per_class", huge=False)


def test_ties_take_the_lowest_index(dev, lib):
    from ytvln import ops
    x = torch.randn(4, 517, generator=torch.Generator().manual_seed(3)).clamp_(max=3.0)
    x[0] = 1.25                                     # a row of equal logits
    x[1, 70] = x[1, 300] = 7.0                      # the maximum twice: thread 70 of wave 1 and thread 44 of wave 0
    x[2, 300] = x[2, 70] = 7.0
    x[2, 516] = 7.0
    x[3] = float("-inf")                            # nothing compares greater than the start value
    t = torch.rand(4, 517, generator=torch.Generator().manual_seed(4))
    loss, score, top = ops.bce_with_logits_rows(x.to(dev), t.to(dev))
    assert top.cpu().tolist() == [0, 70, 70, 0] == torch.argmax(x, 1).tolist()
    want = float(t[0, 0].double() + t[1, 70].double() + t[2, 70].double() + t[3, 0].double())
    assert abs(float(score) - want) <= 1e-6 * want


@pytest.mark.parametrize("kind", ["none", "scalar", "per_class"])
def test_masked_regions_are_exact(dev, lib, kind):
    """x = -10000, t = 0 (what vision_logit holds for padded regions): the term and the gradient are exactly 0."""
    from ytvln import ops
    M, C = 5, 37
    pw = _pos_weight(kind, C)
    pw = None if pw is None else pw.to(dev)
    x = torch.full((M, C), -10000.0, device=dev, requires_grad=True)
    loss, score, top = ops.bce_with_logits_rows(x, torch.zeros(M, C, device=dev), pw, scale=float(C))
    loss.backward()
    assert float(loss) == 0.0 and float(score) == 0.0 and bool((x.grad == 0.0).all()) and top.tolist() == [0] * M
    # open and masked regions side by side: the masked entries add exactly nothing to their row and get exactly no gradient
    xo, to = kernel_inputs(M, 20, seed=9, huge=False)
    xm = torch.cat([xo, torch.full((M, C - 20), -10000.0)], 1).to(dev).requires_grad_(True)
    tm = torch.cat([to, torch.zeros(M, C - 20)], 1).to(dev)
    lm, _, _ = ops.bce_with_logits_rows(xm, tm, pw, scale=float(C))
    lm.backward()
    assert bool((xm.grad[:, 20:] == 0.0).all()) and bool((xm.grad[:, :20] != 0.0).any())
    ref, _, _ = bce_rows_ref(xo, to, None if pw is None else pw[:20].cpu(), scale=20.0)          # sum over the open regions / M
    close(lm, ref, 2e-6, 2e-6, "open regions only")


def test_nan_propagates_to_the_loss_and_stays_in_its_row(dev, lib):
    from ytvln import ops
    x, t = kernel_inputs(6, 300, seed=11)
    x = x.clone()
    x[2, 17] = float("nan")
    xg = x.to(dev).requires_grad_(True)
    loss, score, top = ops.bce_with_logits_rows(xg, t.to(dev), scale=300.0)
    loss.backward()
    assert bool(torch.isnan(loss))
    rows = [0, 1, 3, 4, 5]
    assert bool(torch.isfinite(xg.grad[rows]).all()) and bool((xg.grad[rows].abs().sum(1) > 0).all())
    assert torch.equal(top.cpu()[rows], torch.argmax(x[rows], 1)) and 0 <= int(top[2]) < 300


def test_the_old_entry_point_keeps_its_cap_and_agrees_on_small_inputs(dev, lib):
    from ytvln import ops
    x, t = _inputs(33, 3129)
    with pytest.raises(RuntimeError, match="ytvln_bce_fwd_f32 failed"):
        ops.bce_with_logits(x.to(dev), t.to(dev))
    loss, _, _ = ops.bce_with_logits_rows(x.to(dev), t.to(dev))
    assert bool(torch.isfinite(loss))
    xs, ts = kernel_inputs(8, 16, seed=13, huge=False)
    ts = torch.rand(8, 16, generator=torch.Generator().manual_seed(14))
    for pw in (None, torch.tensor([3.0], device=dev)):
        old = ops.bce_with_logits(xs.to(dev), ts.to(dev), pw)
        new, _, _ = ops.bce_with_logits_rows(xs.to(dev), ts.to(dev), pw, scale=1.0)
        print(f"[bce rows vs flat 8x16 pw={pw is not None}] {float(new):.9g} vs {float(old):.9g}")
        close(new, old, 1e-6, 1e-6, "rows against the flat kernel")


def test_two_calls_give_the_same_bits(dev, lib):
    from ytvln import ops
    x, t = _inputs(300, 259)
    pw = _pos_weight("per_class", 259).to(dev)
    res = []
    for _ in range(2):
        xg = x.to(dev).requires_grad_(True)
        loss, score, top = ops.bce_with_logits_rows(xg, t.to(dev), pw, scale=259.0)
        loss.backward()
        res.append((loss.detach().clone(), score.clone(), top.clone(), xg.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*res))


def test_forward_and_backward_capture_into_one_graph(dev, lib):
    """Replayed on new input contents the graph gives what an eager run on those contents gives, bit for bit."""
    from ytvln import ops
    M, C = 37, 300
    x0, t0 = kernel_inputs(M, C, seed=21)
    x1, t1 = kernel_inputs(M, C, seed=22)
    x, t = x0.to(dev).requires_grad_(True), t0.to(dev)
    pw = _pos_weight("per_class", C).to(dev)
    g = torch.tensor(0.5, device=dev)

    def run():
        loss, score, top = ops.bce_with_logits_rows(x, t, pw, scale=float(C))
        return (loss.detach(), score, top) + torch.autograd.grad(loss, [x], g)

    # (code objects loaded before the capture.  Detached results only: a live autograd graph from this eager run would keep x's gradient
    #  accumulator, which is bound to the stream it was made on, and the captured backward would then wait on that stream from inside the capture)
    first = [a.clone() for a in run()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    with torch.no_grad():
        x.copy_(x1)
        t.copy_(t1)
        g.fill_(2.0)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [a.clone() for a in captured]
    eager = run()
    torch.cuda.synchronize()
    assert len(replayed) == 4
    for i, (a, e) in enumerate(zip(replayed, eager)):
        assert torch.equal(a, e), i
    assert not torch.equal(replayed[0], first[0]) and not torch.equal(replayed[3], first[3])
    ref, _, ref_top = bce_rows_ref(x1, t1, pw.cpu(), scale=float(C))          # and it is the new contents that were used
    close(replayed[0], ref, 2e-6, 2e-6, "replayed loss")
    assert torch.equal(replayed[2].cpu(), ref_top)


# ---- model level: micro configuration, every dropout off ------------------------------------------------------------------------------
def _targets(task, v_logit_loss, mask, seed=77):
    """CPU targets for the micro batch (N = 3 pairs, 7 labels, 10 regions of which `mask` marks the real ones)."""
    rs = np.random.RandomState(seed)
    N, R = mask.shape
    if task == "VL-classifier":
        t = np.where(rs.random_sample((N, NUM_LABELS)) < 0.35, rs.choice([0.3, 0.6, 0.9, 1.0], (N, NUM_LABELS)), 0.0)
        return torch.from_numpy(t.astype(np.float32))
    if task == "VL-logit":
        return torch.tensor([1])
    if task == "VL-binary-classifier":
        return torch.tensor([1, 0, 1])
    if v_logit_loss == "bce":
        t = (rs.random_sample((N, R)) < 0.3) & (mask != 0)
        t[:, 0] = True
        return torch.from_numpy(t.astype(np.float32)).unsqueeze(2)
    p = rs.random_sample((N, R)) * (mask != 0)
    return torch.from_numpy((p / p.sum(1, keepdims=True)).astype(np.float32))


def _micro_pair(dev, bs=None, seed=None):
    """(GPU model in training mode, its inputs on the device, fp64 state, oracle config, the inputs on the CPU, region mask)."""
    import vilbert_ref as O
    from ytvln import synth
    if bs is None:
        mask = gold("g21_vltasks_micro.npz")["region_mask"]
        nb = synth.make_batch(**MICRO_BATCH)
    else:
        nb = synth.make_batch(**{**MICRO_BATCH, "bs": bs, "seed": seed})
        mask = np.ones((bs, MICRO_BATCH["frames"] * MICRO_BATCH["boxes"]), dtype=gold("g21_vltasks_micro.npz")["region_mask"].dtype)
        mask[1, -3:] = 0
        mask[bs - 1, -1:] = 0
    model = build_model("micro.json", "mul")
    W = make_weights(model, 41)
    model.load_state_dict(state_of(W))
    cfg = O.RefConfig(**cfg_dict("micro.json", fusion_method="mul", **ZERO_DROP))
    return model.to(dev).train(), inputs_of(nb, mask, dev), state_of(W, torch.float64), cfg, inputs_of(nb, mask), mask


NOISE = 1e-7          # the absolute size tests/test_vltasks_gpu.py holds an identically-zero gradient to (its NOISE)
KEY_BIASES = ("key.bias", "key1.bias", "key2.bias")


def _identically_zero(task, kw):
    """Name test of the tensors whose gradient is zero for every input, so that no relative statistic exists: the attention key biases
    (test_vltasks_gpu._is_noise: a constant added to every key's score of a query leaves the softmax unchanged) and, where the loss is
    a softmax over the very logits a tensor shifts by one common amount, that tensor -- vil_logit.bias under "VL-logit" (softmax over the
    options), and under the KL of "V-logit" (softmax over the regions) vision_logit.bias and the bias of the last image-side LayerNorm,
    which moves every region's logit by the same vision_logit.weight . bias.  Nothing else is excluded from the relative bar."""
    extra = {"VL-logit": ("vil_logit.bias",), "V-logit-kl": ("vision_logit.bias", "bert.encoder.v_layer.1.output.LayerNorm.bias")}
    names = extra.get(task if task != "V-logit" else "V-logit-" + kw["v_logit_loss"], ())
    return lambda k: k.endswith(KEY_BIASES) or k in names


def _zero_bound(name, task, num_options=None):
    """What an identically-zero gradient is held to: NOISE.  One tensor cannot meet that in fp32 for a reason outside this change:
    vil_logit.bias under "VL-logit" receives sum_i (p_i - y_i) of ONE row of ytvln_ce_bwd_f32, p_i = expf(x_i - lse) with lse in [1, 2)
    here (log 3 + 0.01).  The rounding of lse moves every p_i the same way, by up to half an ulp of lse = 2^-24 relative, so up to 2^-24 on
    the sum (which is 1); the rounding of each x_i - lse does the same once more on average; expf and the subtraction of y_i are good to
    an ulp of p_i < 0.5, 2^-25, each: 2^-24 + 2^-24 + 2 K 2^-25 for K options (K = 3: 3.0e-7), where the mean over several rows or
    terms of 1e-2 (the other tensors above) stay far below NOISE."""
    if name == "vil_logit.bias" and task == "VL-logit":
        return 2.0 ** -24 + 2.0 ** -24 + 2 * num_options * 2.0 ** -25
    return NOISE


TASK_CASES = [("VL-classifier", {}), ("VL-logit", {"num_options": 3}), ("VL-binary-classifier", {}), ("V-logit", {"v_logit_loss": "bce"}),
              ("V-logit", {"v_logit_loss": "kl"})]


@pytest.mark.parametrize("task,kw", TASK_CASES, ids=[c[0] + "".join("-" + str(v) for v in c[1].values()) for c in TASK_CASES])
def test_task_loss_on_the_micro_model(dev, lib, task, kw):
    from ytvln import vl_tasks
    model, inp, S, cfg, inp_cpu, mask = _micro_pair(dev)
    target = _targets(task, kw.get("v_logit_loss"), mask)
    loss, score, n = vl_tasks.task_loss(task, model(*inp), target.to(dev), **kw)
    loss.backward()
    names = [k for k, _ in model.named_parameters()]
    leaves = {k: S[k].requires_grad_(True) for k in names}
    ref, ref_score = task_loss_ref(task, vltasks_forward(S, cfg, *inp_cpu), target, **kw)
    ref.backward()
    print(f"[vl task {task} {kw}] loss {float(loss):.7f} vs {float(ref):.7f}, score {float(score)} vs {float(ref_score)}, batch {n}")
    assert n == (1 if task == "VL-logit" else 3) and loss.dtype == torch.float32 and loss.is_cuda and score.is_cuda and score.shape == ()
    assert abs(float(loss) - float(ref)) <= 1e-4
    assert float(score) == float(ref_score)
    grads = dict(model.named_parameters())
    # a tensor the loss does not depend on has no gradient (or an exactly zero one); every other tensor has one
    assert all(grads[k].grad is not None for k in names if leaves[k].grad is not None)
    assert all(grads[k].grad is None or not bool(grads[k].grad.any()) for k in names if leaves[k].grad is None)
    zero = _identically_zero(task, kw)
    excluded = sorted(k for k in names if leaves[k].grad is not None and zero(k))
    print(f"[vl task {task} {kw}] identically-zero gradients (norm, fp64 norm): "
          + ", ".join(f"{k} {float(grads[k].grad.double().norm()):.2e}/{float(leaves[k].grad.norm()):.2e}" for k in excluded))
    assert all(float(leaves[k].grad.norm()) < 1e-12 for k in excluded)          # fp64 agrees that they are zero
    rels = {k: rel_l2(grads[k].grad, leaves[k].grad) for k in names if leaves[k].grad is not None and not zero(k)}
    small = sorted((k for k in rels if float(leaves[k].grad.norm()) < 1e-6), key=lambda k: float(leaves[k].grad.norm()))
    print(f"[vl task {task} {kw}] gradients of fp64 norm below 1e-6 (fp64 norm, rel-L2): "
          + ", ".join(f"{k} {float(leaves[k].grad.norm()):.2e} {rels[k]:.2e}" for k in small))
    worst = max(rels, key=rels.get)
    print(f"[vl task {task} {kw}] {len(rels)} gradients, worst rel-L2 {rels[worst]:.2e} ({worst}), {len(excluded)} identically zero")
    assert all(float(grads[k].grad.double().norm()) < _zero_bound(k, task, kw.get("num_options")) for k in excluded)
    assert min(float(leaves[k].grad.norm()) for k in rels) > 1e-12
    assert rels[worst] <= 1e-4, (worst, rels[worst])


def _adamw_fp64(S, names, grads, state, step, lr=4e-5, wd=0.01, b1=0.9, b2=0.999, eps=1e-6):
    """The reference's AdamW (denominator sqrt(v) + eps, bias correction in the step size, decay after the update, no-decay tags of
    ytvln.vilbert_init.NO_DECAY, tensors without a gradient skipped) on fp64 leaves."""
    from ytvln.vilbert_init import NO_DECAY
    t = step + 1
    step_size = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    with torch.no_grad():
        for k, g in zip(names, grads):
            if g is None:
                continue
            m, v = state.setdefault(k, (torch.zeros_like(g), torch.zeros_like(g)))
            m.mul_(b1).add_(g, alpha=1.0 - b1)
            v.mul_(b2).addcmul_(g, g, value=1.0 - b2)
            S[k].addcdiv_(m, v.sqrt() + eps, value=-step_size)
            if not any(tag in k for tag in NO_DECAY):
                S[k].add_(S[k], alpha=-lr * wd)


def test_three_task_steps_against_an_fp64_loop(dev, lib):
    from ytvln import vl_tasks
    from ytvln.optimization import AdamW
    from ytvln.vilbert_init import grouped_parameters
    model, inp, S, cfg, inp_cpu, mask = _micro_pair(dev)
    target = _targets("VL-classifier", None, mask)
    batch = tuple(inp) + (target.to(dev),)
    opt = AdamW(grouped_parameters(model, 0.01), lr=4e-5)
    args = args_ns()
    got = [vl_tasks.vl_task_step(model, opt, None, batch, "VL-classifier", args, step=s) for s in range(3)]
    assert opt._arena is not None and all(p.grad is None for p in model.parameters())          # stepped on the arena, gradients dropped
    names = [k for k, _ in model.named_parameters()]
    for k in names:
        S[k].requires_grad_(True)
    state = {}
    for s in range(3):
        ref, ref_score = task_loss_ref("VL-classifier", vltasks_forward(S, cfg, *inp_cpu), target)
        grads = torch.autograd.grad(ref, [S[k] for k in names], allow_unused=True)
        print(f"[vl task step {s}] loss {float(got[s][0]):.7f} vs {float(ref):.7f}, score {float(got[s][1])} vs {float(ref_score)}")
        assert abs(float(got[s][0]) - float(ref)) <= 1e-4 and float(got[s][1]) == float(ref_score)
        assert not got[s][0].requires_grad and got[s][0].is_cuda
        _adamw_fp64(S, names, grads, state, s)
    assert float(got[2][0]) < float(got[0][0])
    worst = 0.0
    for k, p in model.named_parameters():
        a, b = float(p.detach().double().norm()), float(S[k].detach().norm())
        worst = max(worst, abs(a - b) / b)
        assert abs(a - b) <= 2e-6 * b, f"norm after three steps {k}: {a} vs {b}"
    print(f"[vl task step] worst relative parameter-norm error after three steps {worst:.2e}")


def test_two_accumulated_half_batches_equal_one_whole_batch_step(dev, lib):
    """gradient_accumulation_steps = 2: two micro-steps on the halves of a batch, each loss / 2, one optimizer step == one step on the whole
    batch (the loss is a mean over the batch); two optimizer steps, the bar of test_gradient_accumulation_matches_big_batch_of_micro_steps."""
    from ytvln import vl_tasks
    from ytvln.vilbert_init import get_optimization
    args = args_ns(gradient_accumulation_steps=2)
    args.learning_rate = 1e-3
    whole_args = args_ns()
    model, inp, _, _, _, mask = _micro_pair(dev, bs=4, seed=83)
    ref, _, _, _, _, _ = _micro_pair(dev, bs=4, seed=83)
    target = _targets("VL-classifier", None, mask, seed=78).to(dev)
    whole = tuple(inp) + (target,)
    halves = [tuple(a[:2] for a in whole), tuple(a[2:] for a in whole)]
    opt, sched, _, _ = get_optimization(args, model, 10, None)
    ropt, rsched, _, _ = get_optimization(args, ref, 10, None)
    for rep in range(2):
        la = vl_tasks.vl_task_step(model, opt, sched, halves[0], "VL-classifier", args, step=2 * rep)[0]
        lb = vl_tasks.vl_task_step(model, opt, sched, halves[1], "VL-classifier", args, step=2 * rep + 1)[0]
        lw = vl_tasks.vl_task_step(ref, ropt, rsched, whole, "VL-classifier", whole_args, step=rep)[0]
        assert abs(float(la + lb) - float(lw)) <= 1e-5 * abs(float(lw)), (float(la), float(lb), float(lw))
    got = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu()
    want = torch.cat([p.detach().reshape(-1) for p in ref.parameters()]).cpu()
    d = float((got - want).abs().max())
    print(f"[vl task accumulation] max |parameter difference| after two optimizer steps {d:.2e}")
    assert d < 3e-6, d
