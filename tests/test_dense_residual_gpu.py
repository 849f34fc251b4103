"""ops.linear_res / ops.ffn_res with a gradient arriving on the SECOND output (the residual branch that skips the sublayer): the input-gradient
GEMM accumulates into that gradient's buffer (beta = 1), falls back to a buffer of its own when the buffer is one this backward still reads, and
a passthrough node without a residual gradient is the plain op.  fp32 and bf16-resident operands against fp64 autograd on the same (for bf16:
bf16-rounded) operands.

Shapes: M = 150 rows (no multiple of the 32-row tile: a ragged row tail), K = N = 64 (the output gradient and the residual gradient can be one
tensor), I = 96.  Bars: the ones test_kernels_gpu.py::test_linear_and_ffn_autograd (fp32) and
test_bf16_gpu.py::test_linear_ffn_bf16_autograd_and_weight_copies (bf16; a bf16 dx is one more rounding of acc + dr, inside that bar) hold these ops to.
Measured at these shapes: fp32 every relative L2 error <= 3e-7; bf16 y <= 2.3e-3, dx <= 2.9e-3, parameter gradients <= 2.1e-3.

Situation 2 with an activation is the case that used to go wrong: the accumulate rule looked at the activation backward's OUTPUT only, so a residual
gradient that shared its storage with the incoming output gradient was accumulated into (dx right, the caller's gradient buffer overwritten).
LinearFn now hands the rule the incoming gradient as well, as FFNFn always did."""
import pytest
import torch
import torch.nn.functional as F

from helpers import close, rel_l2
from test_kernels_gpu import rnd

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
M, K, I, N = 150, 64, 96, 64
CASES = [("linear_res", None), ("linear_res", "gelu"), ("ffn_res", None)]


@pytest.fixture
def fp32_mode():
    from ytvln import ops
    was = ops.get_matmul_precision()
    ops.set_matmul_precision("fp32")          # fp32 operands stay on the fp32 GEMM; bf16 operands take the bf16-resident path in every mode
    yield
    ops.set_matmul_precision(was)


def _operands(dev, op, bf16):
    x = rnd(dev, 3, M // 3, K, seed=1)
    if op == "ffn_res":
        ps = [rnd(dev, I, K, seed=2, scale=0.2), rnd(dev, I, seed=3), rnd(dev, N, I, seed=4, scale=0.2), rnd(dev, N, seed=5)]
    else:
        ps = [rnd(dev, N, K, seed=2, scale=0.2), rnd(dev, N, seed=3)]
    return (x.to(BF) if bf16 else x), ps


def _reference(op, act, x, ps, dy):
    """fp64 autograd; the weights rounded to bf16 where the kernels read their bf16 copy.  -> (y, dY-part of dx, parameter gradients)."""
    bf16 = x.dtype == BF
    xd = x.detach().double().requires_grad_(True)
    pd = [(p.detach().to(BF) if (bf16 and p.dim() == 2) else p.detach()).double().requires_grad_(True) for p in ps]
    if op == "ffn_res":
        yr = F.linear(F.gelu(F.linear(xd, pd[0], pd[1])), pd[2], pd[3])
    else:
        yr = F.linear(xd, pd[0], pd[1])
        if act == "gelu":
            yr = F.gelu(yr)
    yr.backward(dy.double())
    return yr.detach(), xd.grad, [p.grad for p in pd]


def _run(ops, op, act, x, ps, dy, dr):
    xs = x.clone().requires_grad_(True)
    pl = [p.clone().requires_grad_(True) for p in ps]
    y, r = ops.ffn_res(xs, *pl) if op == "ffn_res" else ops.linear_res(xs, pl[0], pl[1], act)
    if dr is None:
        y.backward(dy)
    else:
        torch.autograd.backward([y, r], [dy, dr])
    torch.cuda.synchronize()
    return y, xs.grad, [p.grad for p in pl]


def _check(what, bf16, y, gx, gps, yr, gx_ref, gps_ref):
    figures = [rel_l2(y, yr), rel_l2(gx, gx_ref)] + [rel_l2(a, b) for a, b in zip(gps, gps_ref)]
    print(f"{what}: rel_l2 y {figures[0]:.3e} dx {figures[1]:.3e} params " + " ".join(f"{v:.3e}" for v in figures[2:]))
    assert gx.dtype == (BF if bf16 else torch.float32) and all(g.dtype == torch.float32 for g in gps), what
    if bf16:
        assert figures[0] < 6e-3, (what, "y", figures[0])
        assert all(v < 1e-2 for v in figures[1:]), (what, figures)
    else:
        close(y, yr, 3e-4, 2e-4, what + " fwd")
        assert all(v < 2e-5 for v in figures[1:]), (what, figures)


@pytest.mark.parametrize("op,act", CASES, ids=["linear", "linear_gelu", "ffn"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_residual_gradient_on_second_output(dev, lib, fp32_mode, precision, op, act):
    from ytvln import ops
    bf16 = precision == "bf16"
    x, ps = _operands(dev, op, bf16)
    dy, dr = rnd(dev, *x.shape[:-1], N, seed=9), rnd(dev, *x.shape, seed=10)
    if bf16:
        dy, dr = dy.to(BF), dr.to(BF)
    yr, gx_ref, gps_ref = _reference(op, act, x, ps, dy)          # one reference: dx is linear in (dY, d residual)
    what = f"{precision} {op} {act}"

    # 1. a fresh contiguous residual gradient: dx = dY-part + dr, written over dr's own buffer (the accumulate path was taken)
    dr1, dy1 = dr.clone(), dy.clone()
    y, gx, gps = _run(ops, op, act, x, ps, dy1, dr1)
    _check(what + " fresh dr", bf16, y, gx, gps, yr, gx_ref + dr.double(), gps_ref)
    assert gx.data_ptr() == dr1.data_ptr(), what + ": dx does not live in the residual gradient's buffer"
    assert torch.equal(dy1, dy), what + ": the output gradient was modified"

    # 2. the residual gradient shares its storage with the output gradient (N = K): no accumulation over an operand, dy untouched
    g = dy.clone()
    y, gx, gps = _run(ops, op, act, x, ps, g, g)
    _check(what + " dr is dy", bf16, y, gx, gps, yr, gx_ref + dy.double(), gps_ref)
    assert torch.equal(g, dy), what + ": the shared gradient buffer was overwritten"

    # 3. no residual gradient on a passthrough node
    y, gx, gps = _run(ops, op, act, x, ps, dy.clone(), None)
    _check(what + " no dr", bf16, y, gx, gps, yr, gx_ref, gps_ref)
