"""CPU: the fp64 restatements of the VL-task losses (tests/vl_task_ref.py) are torch's own losses, the two row-wise BCE entry points
validate their arguments before any launch, and the Python layer refuses CPU tensors and unknown tasks."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from vl_task_ref import bce_rows_ref, kernel_inputs, task_loss_ref


def _outputs(N=6, L=9, R=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    shapes = [(N, L), (N, 1), (N, 2), (N, R, 11), (N, R, 1), (N, 4, 13), (N, 4, 1)]
    return tuple(torch.randn(s, generator=g, dtype=torch.float64) for s in shapes)


def test_restatements_equal_the_torch_losses():
    g = torch.Generator().manual_seed(1)
    outs = _outputs()
    N, L, R = 6, 9, 5
    soft = torch.rand(N, L, generator=g, dtype=torch.float64)
    for pw in (None, torch.tensor([2.5], dtype=torch.float64), torch.rand(L, generator=g, dtype=torch.float64) + 0.5):
        loss, score = task_loss_ref("VL-classifier", outs, soft, pos_weight=pw)
        want = F.binary_cross_entropy_with_logits(outs[0], soft, pos_weight=pw, reduction="none").mean() * L
        assert abs(float(loss - want)) <= 1e-12 * abs(float(want))
        assert float(score) == float(soft.gather(1, outs[0].argmax(1, keepdim=True)).sum())
    tgt = torch.randint(0, 3, (N // 3,), generator=g)
    loss, score = task_loss_ref("VL-logit", outs, tgt, num_options=3)
    assert abs(float(loss - F.cross_entropy(outs[1].view(-1, 3), tgt))) <= 1e-12
    assert float(score) == float((outs[1].view(-1, 3).argmax(1) == tgt).sum())
    tgt = torch.randint(0, 2, (N,), generator=g)
    loss, score = task_loss_ref("VL-binary-classifier", outs, tgt)
    assert abs(float(loss - F.cross_entropy(outs[2], tgt))) <= 1e-12 and float(score) == float((outs[2].argmax(1) == tgt).sum())
    hard = (torch.rand(N, R, 1, generator=g) < 0.4).double()
    loss, score = task_loss_ref("V-logit", outs, hard)
    want = F.binary_cross_entropy_with_logits(outs[4].view(N, R), hard.view(N, R), reduction="none").mean() * R
    assert abs(float(loss - want)) <= 1e-12 * abs(float(want))
    assert float(score) == float((hard.view(N, R).gather(1, outs[4].view(N, R).argmax(1, keepdim=True)) > 0.5).sum())
    dist = torch.softmax(torch.randn(N, R, generator=g, dtype=torch.float64), 1)
    loss, _ = task_loss_ref("V-logit", outs, dist, v_logit_loss="kl")
    want = F.kl_div(F.log_softmax(outs[4].view(N, R), 1), dist, reduction="batchmean")
    assert abs(float(loss - want)) <= 1e-12
    with pytest.raises(KeyError):
        task_loss_ref("VL-nothing", outs, soft)


def test_restatement_on_the_kernel_test_inputs_is_torchs_bce():
    """The recipe of the GPU tests (logits of +-1e4 included): the written-out term is F.binary_cross_entropy_with_logits in fp64."""
    x, t = kernel_inputs(33, 259, seed=5)
    assert float((x.abs() == 1e4).float().mean()) > 0 and 0.01 < float((t > 0).float().mean()) < 0.03
    pw = torch.rand(259, dtype=torch.float64) + 0.5
    loss, score, top = bce_rows_ref(x, t, pw, scale=259.0)
    want = F.binary_cross_entropy_with_logits(x.double(), t.double(), pos_weight=pw) * 259.0
    assert abs(float(loss - want)) <= 1e-12 * abs(float(want))
    assert torch.equal(top, x.argmax(1)) and float(score) == float(t.double()[torch.arange(33), top].sum())


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    from ytvln import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    inf, nan = float("inf"), float("nan")

    def fwd(x=P(16), ldx=8, t=P(16), ldt=8, pw=None, pws=0, scale=1.0, rl=P(16), rh=P(16), rt=P(16), out=P(16), M=4, C=8):
        return lib.ytvln_bce_rows_fwd_f32(x, ldx, t, ldt, pw, pws, scale, rl, rh, rt, out, M, C, None)

    def bwd(x=P(16), ldx=8, t=P(16), ldt=8, pw=None, pws=0, scale=1.0, g=P(16), dx=P(16), lddx=8, M=4, C=8):
        return lib.ytvln_bce_rows_bwd_f32(x, ldx, t, ldt, pw, pws, scale, g, dx, lddx, M, C, None)

    fwd_bad = [dict(x=None), dict(t=None), dict(rl=None), dict(rh=None), dict(rt=None), dict(out=None), dict(M=0), dict(M=-3), dict(C=0),
               dict(C=-1), dict(ldx=7), dict(ldt=7), dict(pw=P(16), pws=2), dict(pws=-1), dict(scale=inf), dict(scale=-inf), dict(scale=nan)]
    bwd_bad = [dict(x=None), dict(t=None), dict(g=None), dict(dx=None), dict(M=0), dict(C=0), dict(ldx=7), dict(ldt=7), dict(lddx=7),
               dict(pw=P(16), pws=2), dict(pws=-1), dict(scale=inf), dict(scale=nan)]
    for fn, cases, tag in ((fwd, fwd_bad, b"bce_rows_fwd"), (bwd, bwd_bad, b"bce_rows_bwd")):
        for kw in cases:
            rc = fn(**kw)
            msg = lib.ytvln_last_error()
            assert rc != 0 and tag in msg and len(msg) > len(tag) + 2, (kw, rc, msg)
    with pytest.raises(RuntimeError, match="ytvln_bce_rows_fwd_f32 failed.*pw_stride"):
        _lib.call("ytvln_bce_rows_fwd_f32", 16, 8, 16, 8, 16, 3, 1.0, 16, 16, 16, 16, 4, 8, None)


def test_cpu_tensors_raise():
    from ytvln import ops, vl_tasks
    x, t = torch.zeros(4, 8), torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bce_with_logits_rows(x, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.bce_with_logits_rows(x, t, torch.ones(8), scale=8.0)
    outs = tuple(o.float() for o in _outputs())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vl_tasks.task_loss("VL-classifier", outs, torch.zeros(6, 9))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vl_tasks.task_loss("V-logit", outs, torch.zeros(6, 5, 1))


def test_unknown_task_and_indivisible_options_raise_key_error():
    from ytvln import vl_tasks
    outs = tuple(o.float() for o in _outputs())
    with pytest.raises(KeyError):
        vl_tasks.task_loss("VL-nothing", outs, torch.zeros(6, 9))
    with pytest.raises(KeyError):
        vl_tasks.task_loss("VL-logit", outs, torch.zeros(1, dtype=torch.long), num_options=4)          # 6 rows, 4 options
    with pytest.raises(KeyError):
        vl_tasks.task_loss("VL-logit", outs, torch.zeros(1, dtype=torch.long))                        # no num_options at all
    with pytest.raises(KeyError):
        vl_tasks.task_loss("V-logit", outs, torch.zeros(6, 5), v_logit_loss="mse")


def test_the_module_does_not_import_the_oracle_and_the_op_returns_three_outputs():
    import inspect
    from ytvln import ops, vl_tasks
    src = inspect.getsource(vl_tasks)
    assert "oracle" not in src and "vilbert_ref" not in src
    assert list(inspect.signature(ops.bce_with_logits_rows).parameters) == ["x", "t", "pos_weight", "scale"]
    assert list(inspect.signature(vl_tasks.task_loss).parameters) == ["task_type", "outputs", "target", "num_options", "v_logit_loss", "pos_weight"]
    assert vl_tasks.TASK_TYPES == ("VL-classifier", "VL-logit", "VL-binary-classifier", "V-logit")
