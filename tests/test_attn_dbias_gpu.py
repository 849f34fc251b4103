"""GPU: the gradient with respect to the per-score attention bias (ytvln_attn_dbias_f32 / _bf16 behind SelfAttentionFn / CoAttentionFn).

The kernel against fp64 autograd at the bars tests/test_attn_bias_gpu.py sets for dq / dk / dv (2e-5 relative L2 in fp32, 2e-2 in bf16) for every
layout of the gradient (nh, n1, 11, the transposed view), ragged / single-query / > 512 sequences, padded head dimensions and the shapes at which
the in-library sum is split into runs; dropout decisions through the identities dq = scale dBias K, dk = scale dBias^T Q and "every row sums to
zero"; the in-library sums against host fp64 sums, bit-reproducible; the autograd plumbing; the modules; the whole model by central differences;
graph capture; and the guard that nothing without a trainable bias reaches the new entry points or changes what it launches."""
import math

import pytest
import torch

from helpers import rel_l2
from test_attn_bias_gpu import _bert_inputs, _co_apply, _lily, _micro_cfg, _ref_connection, make_bias, ref_attention, rnd

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
EPS32 = 2.0 ** -23

# (N, heads, d, Tq, Tk): the issue's list, then two shapes at which the sum over (pair, head) is cut into runs + a workspace pass
# (5 x 4 = 20 problems into a [1,1,..] output; 20 heads into an [N,1,..] output)
_SHAPES = [(2, 4, 8, 6, 5), (1, 3, 32, 33, 65), (2, 2, 64, 1, 95), (2, 8, 128, 33, 95), (2, 12, 64, 60, 60), (2, 8, 128, 80, 288),
           (2, 8, 128, 288, 80), (1, 8, 128, 576, 576), (5, 4, 32, 33, 65), (2, 20, 8, 6, 5)]
_FORMS = ["nh", "n1", "11", "n1T"]


def _raw_dbias(dev, N, heads, d, Tq, Tk, bias, bf, with_mask=True, fwd_bias=True, like=None, seed=1):
    """Forward, backward and the bias-gradient launch of one problem through the raw helpers (any Tq != Tk).  `bias`: the tensor / view the
    forward reads (None: an unbiased problem; then `like` gives the layout of the gradient).  -> (dBias, everything the fp64 reference needs)."""
    from ytvln import ops
    H = heads * d
    A = rnd(dev, N * Tq, 3 * H, seed=seed)
    B = rnd(dev, N * Tk, 3 * H, seed=seed + 1)
    dout = rnd(dev, N * Tq, H, seed=seed + 2)
    if bf:
        A, B, dout = A.to(BF), B.to(BF), dout.to(BF)
    mask = None
    if with_mask:
        mask = torch.zeros(N, Tk, device=dev)
        mask[0, Tk - max(1, Tk // 4):] = -10000.0
    out = torch.empty(N * Tq, H, device=dev, dtype=A.dtype)
    scale = 1 / math.sqrt(d)
    fb = bias if fwd_bias else None
    lse = ops._attn_fwd(A, 0, 3 * H, B, H, 3 * H, B, 2 * H, 3 * H, mask, out, N, heads, Tq, Tk, d, scale, 0.0, None, 0, bias=fb)
    gA, gB = torch.zeros_like(A), torch.zeros_like(B)
    delta = ops._attn_bwd(A, 0, 3 * H, B, H, 3 * H, B, 2 * H, 3 * H, mask, out, dout, lse, gA, 0, 3 * H, gB, H, 3 * H, gB, 2 * H, 3 * H,
                          N, heads, Tq, Tk, d, scale, 0.0, None, 0, bias=fb)
    pr = ops._attn_problem(A, 0, 3 * H, B, H, 3 * H, B, 2 * H, 3 * H, mask, Tq, Tk, 0.0, 0, ctx_in=out, dctx=dout, lse_in=lse, delta=delta)
    like = like or (tuple(bias.shape), torch.float32)
    g = ops._attn_dbias(pr, fb, like, bf, N, heads, Tq, Tk, d, scale, None, dev)
    return g, (A, B, dout, mask)


def _ref_dbias(N, heads, d, Tq, Tk, bias, ops_in):
    """fp64 autograd: the gradient of the tensor / view `bias` ([N or 1, heads or 1, Tq, Tk]) itself"""
    A, B, dout, mask = ops_in
    H = heads * d
    b64 = bias.detach().double().requires_grad_()
    q, k, v = A[:, :H].double().view(N, Tq, H), B[:, H:2 * H].double().reshape(N, Tk, H), B[:, 2 * H:].double().reshape(N, Tk, H)
    ref, _ = ref_attention(q, k, v, None if mask is None else mask.double(), b64.expand(N, heads, Tq, Tk), heads)
    ref.backward(dout.double().view(N, Tq, H))
    return b64.grad


def _kernel_case(dev, N, heads, d, Tq, Tk, form, bf, with_mask=True):
    bias, _ = make_bias(dev, form, N, heads, Tq, Tk)
    g, ins = _raw_dbias(dev, N, heads, d, Tq, Tk, bias, bf, with_mask)
    ref = _ref_dbias(N, heads, d, Tq, Tk, bias, ins)
    assert g.shape == bias.shape == ref.shape and g.dtype == torch.float32
    err = rel_l2(g, ref)
    print(f"attn dbias {'bf16' if bf else 'fp32'} N{N} h{heads} d{d} Tq{Tq} Tk{Tk} {form} mask {with_mask}: rel l2 {err:.2e}")
    assert bool(torch.isfinite(g).all())
    ninf = torch.isinf(bias)
    assert float(g[ninf].abs().max() if bool(ninf.any()) else 0.0) == 0.0, "entries under a -inf bias get exactly 0"
    assert err < (2e-2 if bf else 2e-5), err


@pytest.mark.parametrize("form", _FORMS)
@pytest.mark.parametrize("N,heads,d,Tq,Tk", _SHAPES)
def test_dbias_fp32_against_fp64_autograd(dev, lib, N, heads, d, Tq, Tk, form):
    _kernel_case(dev, N, heads, d, Tq, Tk, form, bf=False)


@pytest.mark.parametrize("form", _FORMS)
@pytest.mark.parametrize("N,heads,d,Tq,Tk", [s for s in _SHAPES if s[2] in (64, 128)])
def test_dbias_bf16_against_fp64_autograd(dev, lib, N, heads, d, Tq, Tk, form):
    _kernel_case(dev, N, heads, d, Tq, Tk, form, bf=True)


@pytest.mark.parametrize("bf", [False, True])
def test_dbias_without_key_mask_and_with_a_null_forward_bias(dev, lib, bf):
    _kernel_case(dev, 2, 12, 64, 60, 60, "nh", bf, with_mask=False)
    _kernel_case(dev, 2, 8, 128, 33, 95, "n1", bf, with_mask=False)
    # a zero bias requiring grad on an otherwise UNBIASED problem: the forward / backward ran without a bias record (the unbiased kernels),
    # the gradient launch gets NULL for the forward values and only the layout of the gradient
    for with_mask in (True, False):
        N, heads, d, Tq, Tk = 2, 8, 128, 33, 95
        zero = torch.zeros(N, 1, Tq, Tk, device=dev)
        g, ins = _raw_dbias(dev, N, heads, d, Tq, Tk, zero, bf, with_mask, fwd_bias=False)
        err = rel_l2(g, _ref_dbias(N, heads, d, Tq, Tk, zero, ins))
        print(f"attn dbias null forward bias bf16 {bf} mask {with_mask}: rel l2 {err:.2e}")
        assert err < (2e-2 if bf else 2e-5)


# ---- dropout: the decisions are the forward's ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("N,T,heads,d", [(2, 80, 12, 64), (2, 95, 4, 128)])
def test_dropout_decisions_match_the_backward_kernels(dev, lib, bf, p, N, T, heads, d):
    """One SelfAttentionFn backward with a trainable [N,h,T,T] bias.  dq and dk come from the EXISTING kernels under the same rng record, and
    dS is the only thing they share with dBias: dq = scale dBias K, dk = scale dBias^T Q (host fp64, from the returned dBias; bars 2e-5 / 2e-2).
    A wrong element index of the hash or a wrong decode of the stored keep bits breaks both, and the row sums:
        sum_j dS_ij = sum_j p_ij keep_ij/(1-p) dp_ij - delta_i sum_j p_ij = dO_i.O_i - delta_i = 0.
    Bound on |sum_j dBias_ij|, per row, with A = sum_j |dBias_ij| and B = sum_c |dO_ic O_ic| (>= |delta_i| = sum_j p_ij |delta_i|, the other side
    of the cancellation in every term):  Tk eps32 (A + B) -- Tk terms, each a handful of fp32 roundings relative to its two cancelling parts
    (exp of an argument of magnitude <= ~20 alone is ~10 eps), far below what one wrong decision costs (p_ij dp_ij / (1-p), i.e. O(A / Tk)).
    bf16: the forward rounds the dropped-out probabilities and the context it stores to bf16 (relative 2^-9 each, round to nearest), so
    dO.O_stored - sum_j P~_ij dp_ij is up to 2^-9 sum_j P~_ij |dp_ij| + 2^-9 B, and P~ dp = dS + p delta gives sum_j P~_ij |dp_ij| <= A + B:
    the bf16 bound adds 2^-9 A + 2^-8 B."""
    from ytvln import ops
    H = heads * d
    st = ops.DropoutState(dev) if p > 0 else None
    qkv = rnd(dev, N * T, 3 * H, seed=5).to(BF if bf else torch.float32).requires_grad_()
    mask = torch.zeros(N, T, device=dev)
    mask[0, T - 9:] = -10000.0
    bias = make_bias(dev, "nh", N, heads, T, T, seed=3)[0].requires_grad_()
    out, _ = ops.SelfAttentionFn.apply(qkv, mask, N, T, heads, p, st.tensor if st else None, 9, bias)
    dout = rnd(dev, N * T, H, seed=6).to(out.dtype)
    out.backward(dout)
    dB = bias.grad.double()
    assert tuple(dB.shape) == (N, heads, T, T) and bool(torch.isfinite(dB).all())
    heads_of = lambda x: x.double().view(N, T, heads, d).permute(0, 2, 1, 3)          # noqa: E731
    q, k = heads_of(qkv.detach()[:, :H]), heads_of(qkv.detach()[:, H:2 * H])
    dq, dk = heads_of(qkv.grad[:, :H]), heads_of(qkv.grad[:, H:2 * H])
    eq, ek = rel_l2(dq, dB @ k / math.sqrt(d)), rel_l2(dk, dB.transpose(-1, -2) @ q / math.sqrt(d))
    A = dB.abs().sum(-1)
    Bq = (heads_of(dout) * heads_of(out.detach())).abs().sum(-1)
    bound = T * EPS32 * (A + Bq) + ((2.0 ** -9) * A + (2.0 ** -8) * Bq if bf else 0.0)
    rows = dB.sum(-1).abs()
    print(f"attn dbias dropout p {p} bf16 {bf} T{T} d{d}: dq {eq:.2e} dk {ek:.2e} worst row sum / bound {float((rows / bound).max()):.3f}")
    assert eq < (2e-2 if bf else 2e-5) and ek < (2e-2 if bf else 2e-5), (eq, ek)
    assert bool((rows <= bound).all()), float((rows / bound).max())
    if p > 0:          # the decisions really were drawn: about p of the unmasked scores carry dS = -p delta only; here: dBias differs from a p = 0 run
        qkv2 = qkv.detach().clone().requires_grad_()
        b2 = bias.detach().clone().requires_grad_()
        o2, _ = ops.SelfAttentionFn.apply(qkv2, mask, N, T, heads, 0.0, None, 9, b2)
        o2.backward(dout)
        assert rel_l2(b2.grad, dB) > 0.05


# ---- reductions ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("N,heads,d,Tq,Tk", [(2, 8, 128, 80, 288), (2, 12, 64, 60, 60), (5, 4, 64, 33, 65), (2, 20, 64, 6, 5)])
def test_in_library_sums_equal_host_sums_and_are_reproducible(dev, lib, bf, N, heads, d, Tq, Tk):
    """[N,1,..] / [1,1,..] gradients = the fp64 host sum of the [N,h,..] gradient over the reduced dimensions (2e-5: fp32 accumulation of at most
    N x heads terms), with and without the workspace pass ((5,4,..) into 11 and 20 heads into n1 are split into runs); two runs bit-identical."""
    from ytvln import _lib
    import ctypes
    full = torch.zeros(N, heads, Tq, Tk, device=dev)
    nh, _ = _raw_dbias(dev, N, heads, d, Tq, Tk, full, bf)
    split = []
    for shape, dims in (((N, 1, Tq, Tk), (1,)), ((1, 1, Tq, Tk), (0, 1))):
        z = torch.zeros(shape, device=dev)
        g1, _ = _raw_dbias(dev, N, heads, d, Tq, Tk, z, bf)
        g2, _ = _raw_dbias(dev, N, heads, d, Tq, Tk, z, bf)
        assert torch.equal(g1, g2), "bit-reproducible"
        err = rel_l2(g1, nh.double().sum(dims, keepdim=True))
        rec = _lib.AttnBias()
        rec.ptr, rec.stride_q, rec.stride_k = 64, Tk, 1
        rec.stride_n = Tq * Tk if shape[0] > 1 else 0
        split.append(lib.ytvln_attn_dbias_chunks(ctypes.addressof(rec), N, heads, Tq, Tk))
        print(f"attn dbias sum over {dims} N{N} h{heads} Tq{Tq} Tk{Tk} bf16 {bf}: rel l2 {err:.2e} runs {split[-1]}")
        assert err < 2e-5, err
    a, _ = _raw_dbias(dev, N, heads, d, Tq, Tk, full, bf)
    assert torch.equal(a, nh)
    if (N, heads) == (5, 4):
        assert split == [1, 5]
    if heads == 20:
        assert split[0] == 5 and split[1] > 1


# ---- autograd plumbing -----------------------------------------------------------------------------------------------------------------------
def _self_apply(dev, bias, N=2, T=33, heads=4, d=32, bf=False, qkv_grad=True):
    from ytvln import ops
    H = heads * d
    qkv = rnd(dev, N * T, 3 * H, seed=5).to(BF if bf else torch.float32).requires_grad_(qkv_grad)
    mask = torch.zeros(N, T, device=dev)
    mask[0, T - 5:] = -10000.0
    out, lse = ops.SelfAttentionFn.apply(qkv, mask, N, T, heads, 0.0, None, 0, bias)
    dout = rnd(dev, N * T, H, seed=6).to(out.dtype)
    return qkv, mask, out, dout


def _self_ref(qkv, mask, dout, dense64, N, T, heads, d):
    H = heads * d
    x = qkv.detach().double()
    ref, _ = ref_attention(x[:, :H].reshape(N, T, H), x[:, H:2 * H].reshape(N, T, H), x[:, 2 * H:].reshape(N, T, H), mask.double(), dense64, heads)
    ref.backward(dout.double().view(N, T, H))


def test_expanded_parameter_gets_the_sum_over_pairs(dev, lib):
    """A [1,h,T,T] parameter expanded to [N,h,T,T] (stride 0, size > 1): the library returns the full [N,h,T,T] gradient, autograd's
    expand-backward sums it over pairs."""
    N, T, heads, d = 3, 33, 4, 32
    par = (torch.randn(1, heads, T, T, generator=torch.Generator().manual_seed(2)) * 2).to(dev).requires_grad_()
    qkv, mask, out, dout = _self_apply(dev, par.expand(N, heads, T, T), N, T, heads, d)
    out.backward(dout)
    p64 = par.detach().double().requires_grad_()
    _self_ref(qkv, mask, dout, p64.expand(N, heads, T, T), N, T, heads, d)
    assert par.grad.shape == par.shape and rel_l2(par.grad, p64.grad) < 2e-5


@pytest.mark.parametrize("bf", [False, True])
def test_shared_transposed_co_attention_mask_receives_both_directions(dev, lib, bf):
    """CoAttentionFn with (co^T view, co) of ONE [N,1,R,T] leaf: each direction's gradient is computed in its own layout, the leaf receives the
    sum (the transposed view's through autograd's transpose-backward)."""
    N, R, T, heads, d = 2, 72, 20, 2, 64
    Hb = heads * d
    co = make_bias(dev, "n1", N, heads, R, T, seed=21)[0].requires_grad_()
    got, (q1, kv1, q2, kv2, m1, m2, g1, g2) = _co_apply(dev, bf, 0.0, (co.transpose(2, 3), co), N=N, R=R, T=T, heads=heads, d=d)
    c64 = co.detach().double().requires_grad_()
    x = [t.detach().double() for t in (q1, kv1, q2, kv2)]
    r1, _ = ref_attention(x[2].view(N, T, Hb), x[1][:, :Hb].reshape(N, R, Hb), x[1][:, Hb:].reshape(N, R, Hb), m1.double(),
                          c64.transpose(2, 3).expand(N, heads, T, R), heads)
    r2, _ = ref_attention(x[0].view(N, R, Hb), x[3][:, :Hb].reshape(N, T, Hb), x[3][:, Hb:].reshape(N, T, Hb), m2.double(),
                          c64.expand(N, heads, R, T), heads)
    torch.autograd.backward([r1, r2], [g1.double().view(N, T, Hb), g2.double().view(N, R, Hb)])
    err = rel_l2(co.grad, c64.grad)
    print(f"attn dbias shared co-attention mask bf16 {bf}: rel l2 {err:.2e}")
    assert co.grad.shape == co.shape and err < (2e-2 if bf else 2e-5)


def test_one_live_direction_and_constant_biases(dev, lib):
    """Only ctx1 reaches the loss: bias1 gets its gradient, bias2 -- whose context gradient is None -- gets None; and the other way round.
    A bias that does not require grad gets None and no dbias launch."""
    from ytvln import ops
    N, R, T, heads, d = 2, 40, 20, 2, 64
    Hb = heads * d
    for live in (0, 1):
        b1 = make_bias(dev, "n1", N, heads, T, R, seed=4)[0].requires_grad_()
        b2 = make_bias(dev, "nh", N, heads, R, T, seed=5)[0].requires_grad_()
        q1, kv1, q2, kv2 = (rnd(dev, N * n_, w * Hb, seed=11 + i).requires_grad_() for i, (n_, w) in enumerate(((R, 1), (R, 2), (T, 1), (T, 2))))
        m1, m2 = torch.zeros(N, R, device=dev), torch.zeros(N, T, device=dev)
        outs = ops.CoAttentionFn.apply(q1, kv1, q2, kv2, m1, m2, N, R, T, heads, 0.0, 0.0, None, 3, 4, b1, b2)
        g = rnd(dev, *outs[live].shape, seed=8)
        names = _spy(lambda: outs[live].backward(g))
        assert [n for n in names if "dbias" in n] == ["ytvln_attn_dbias_f32"]
        alive, dead = ((b1, b2), (b2, b1))[live]
        assert dead.grad is None and alive.grad is not None and alive.grad.shape == alive.shape
        x = [t.detach().double() for t in (q1, kv1, q2, kv2)]
        a64 = alive.detach().double().requires_grad_()
        if live == 0:
            r, _ = ref_attention(x[2].view(N, T, Hb), x[1][:, :Hb].reshape(N, R, Hb), x[1][:, Hb:].reshape(N, R, Hb), m1.double(),
                                 a64.expand(N, heads, T, R), heads)
        else:
            r, _ = ref_attention(x[0].view(N, R, Hb), x[3][:, :Hb].reshape(N, T, Hb), x[3][:, Hb:].reshape(N, T, Hb), m2.double(),
                                 a64.expand(N, heads, R, T), heads)
        r.backward(g.double().view(r.shape))
        assert rel_l2(alive.grad, a64.grad) < 2e-5
    # constant bias: no gradient, no launch
    const = make_bias(dev, "n1", 2, 4, 33, 33)[0]
    qkv, mask, out, dout = _self_apply(dev, const)
    assert [n for n in _spy(lambda: out.backward(dout)) if "dbias" in n] == [] and const.grad is None and qkv.grad is not None
    # trainable bias, constant qkv: the bias gradient alone
    b = make_bias(dev, "n1", 2, 4, 33, 33)[0].requires_grad_()
    qkv, mask, out, dout = _self_apply(dev, b, qkv_grad=False)
    out.backward(dout)
    assert b.grad is not None and qkv.grad is None


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float64])
def test_bias_dtype_round_trip(dev, lib, dt):
    """A bf16 / fp64 bias is read as fp32 and receives a gradient of its own dtype: the fp32 result converted once (bf16: one rounding, 2^-9)."""
    N, T, heads, d = 2, 33, 4, 32
    b32 = make_bias(dev, "n1", N, heads, T, T)[0]
    b = b32.to(dt).requires_grad_()
    qkv, mask, out, dout = _self_apply(dev, b, N, T, heads, d)
    out.backward(dout)
    ref = b.detach().float().requires_grad_()          # the values the launches read
    qkv2, _, out2, _ = _self_apply(dev, ref, N, T, heads, d)
    out2.backward(dout)
    assert b.grad.dtype == dt and b.grad.shape == b.shape
    assert torch.equal(b.grad, ref.grad.to(dt))


# ---- modules ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,T", [(5, 6), (70, 45)])
def test_modules_with_a_trainable_mask(dev, lib, R, T):
    """BertSelfAttention (T tokens), BertImageSelfAttention (R regions) and a connection layer (R x T co_attention_mask), each with a mask that
    requires grad, against the fp64 restatement on the module's own weights (test_biattention_with_co_attention_mask's); the mask's gradient
    at the bar that file's module tests hold gradients to (rel-L2 <= 1e-4)."""
    from ytvln.vilbert import BertConnectionLayer, BertImageSelfAttention, BertSelfAttention
    cfg = _micro_cfg()
    torch.manual_seed(0)
    N = 3
    for cls, hidden, heads, L in ((BertSelfAttention, cfg.hidden_size, cfg.num_attention_heads, T),
                                  (BertImageSelfAttention, cfg.v_hidden_size, cfg.v_num_attention_heads, R)):
        m = cls(cfg).to(dev).eval()
        for form in ("n1", "nh", "11"):
            mask = make_bias(dev, form, N, heads, L, L, seed=9)[0].requires_grad_()
            x = rnd(dev, N, L, hidden, seed=3).requires_grad_()
            out, _ = m(x, mask)
            gy = rnd(dev, N, L, hidden, seed=4)
            out.backward(gy)
            W = {k: v.detach().double() for k, v in m.named_parameters()}
            xd, m64 = x.detach().double().requires_grad_(), mask.detach().double().requires_grad_()
            q, k, v = (xd @ W[f"{n}.weight"].t() + W[f"{n}.bias"] for n in ("query", "key", "value"))
            ref, _ = ref_attention(q, k, v, None, m64.expand(N, heads, L, L), heads)
            ref.backward(gy.double())
            e = rel_l2(mask.grad, m64.grad)
            print(f"{cls.__name__} L{L} {form}: mask grad rel l2 {e:.2e}")
            assert mask.grad.shape == mask.shape and e < 1e-4 and rel_l2(x.grad, xd.grad) < 1e-4
    layer = BertConnectionLayer(cfg).to(dev).eval()
    heads = cfg.bi_num_attention_heads
    N = 4
    x1, x2 = rnd(dev, N, R, cfg.v_hidden_size, seed=1), rnd(dev, N, T, cfg.hidden_size, seed=2)
    m1, m2 = torch.zeros(N, 1, 1, R, device=dev), torch.zeros(N, 1, 1, T, device=dev)
    m1[0, ..., R - 2:] = -10000.0
    m2[1, ..., T - 3:] = -10000.0
    co = make_bias(dev, "n1", N, heads, R, T, seed=5)[0].requires_grad_()
    c1, c2, _ = layer.biattention(x1, m1, x2, m2, co, True)
    g1, g2 = rnd(dev, *c1.shape, seed=6), rnd(dev, *c2.shape, seed=7)
    torch.autograd.backward([c1, c2], [g1, g2])
    c64 = co.detach().double().requires_grad_()
    r1, r2, _, _ = _ref_connection(layer, x1.double(), m1.double(), x2.double(), m2.double(), c64, heads)
    torch.autograd.backward([r1, r2], [g1.double(), g2.double()])
    e = rel_l2(co.grad, c64.grad)
    print(f"BertBiAttention R{R} T{T}: co_attention_mask grad rel l2 {e:.2e}")
    assert co.grad.shape == co.shape and e < 1e-4


# ---- whole model -----------------------------------------------------------------------------------------------------------------------------
_FD_STEP = 1e-2


def _directional(loss_fn, x, direction, grad):
    """(central difference along `direction`, <grad, direction>) of loss_fn at x (x is modified in place and restored)"""
    base = x.detach().clone()
    with torch.no_grad():
        x.copy_(base + _FD_STEP * direction)
        lp = loss_fn()
        x.copy_(base - _FD_STEP * direction)
        lm = loss_fn()
        x.copy_(base)
    return (lp - lm) / (2 * _FD_STEP), float((grad.double() * direction.double()).sum())


def _model_check(dev):
    from ytvln import ops
    model, cfg = _lily(dev)
    bert = next(m for m in model.modules() if type(m).__name__ == "BertModel").eval()
    ids, feats, loc, am, vm, co = _bert_inputs(dev, R=5)
    co = (co + 0.25 * rnd(dev, *co.shape, seed=12)).requires_grad_()
    bert.encoder.use_co_attention_mask = True
    w = None

    def loss():
        nonlocal w
        a, b = bert(ids, feats, loc, None, am, vm, co)[:2]
        if w is None:
            w = (rnd(dev, *a.shape, seed=21).double(), rnd(dev, *b.shape, seed=22).double())
        return (a.double() * w[0]).sum() + (b.double() * w[1]).sum()

    qw = bert.encoder.c_layer[0].biattention.query1.weight
    L = loss()
    gco, gq = torch.autograd.grad(L, (co, qw))
    unit = lambda t, s: (lambda v: v / v.norm())(rnd(dev, *t.shape, seed=s, scale=1.0))          # noqa: E731
    f = lambda: float(loss())          # noqa: E731
    fd_co, an_co = _directional(f, co, unit(co, 31), gco)
    fd_q, an_q = _directional(f, qw, unit(qw, 32), gq)
    # two-stream mode: the same gradient bit for bit
    tsp = ops.get_two_stream()
    ops.set_two_stream(not tsp)
    try:
        gco2, = torch.autograd.grad(loss(), (co,))
    finally:
        ops.set_two_stream(tsp)
    return co, gco, gco2, abs(fd_co - an_co) / abs(an_co), abs(fd_q - an_q) / abs(an_q)


def test_whole_model_gradient_of_the_co_attention_mask(dev, lib):
    """tiny_2_2_1, eval mode, encoder.use_co_attention_mask = True, co_attention_mask [N,R,T] requiring grad (through BertModel's `* 5.0`, the
    unsqueeze and each connection layer's transposed view): the gradient is finite, has the input's shape, is the same bit for bit with
    two-stream mode toggled, and agrees with a central difference (step 1e-2) along a fixed random unit direction.  The tolerance of that check
    is not chosen freely: the same check on query1.weight of the first connection layer -- a gradient the code produced before this feature --
    measures what fp32 forward passes and the step's truncation leave; three times that deviation is the bar (the margin covers the different
    curvature along the two directions).
    Measured on an MI355X: query1.weight deviation 7.078e-03 (bar: 2.12e-02), co_attention_mask deviation 7.790e-04 (both relative to the analytic
    value; the forward kernels are deterministic, so the figures repeat)."""
    co, g, g2, dev_co, dev_q = _model_check(dev)
    print(f"whole model directional check: co_attention_mask {dev_co:.3e}, query1.weight {dev_q:.3e}")
    assert g.shape == co.shape and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert torch.equal(g, g2)
    assert dev_co <= 3 * _Q_DEVIATION, (dev_co, dev_q)


_Q_DEVIATION = 7.078e-3          # the measured query1.weight deviation (see the docstring above)


# ---- capture ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("form,N,heads", [("n1", 2, 4), ("11", 5, 4)])
def test_graph_capture_replays_bit_equal(dev, lib, bf, form, N, heads):
    """Forward + backward of SelfAttentionFn with a trainable bias (with dropout; 11 over 20 problems takes the workspace pass) captured by
    torch.cuda.graph: the replay equals the eager run bit for bit -- context, dqkv and dBias."""
    from ytvln import ops
    T, d, p = 65, 64, 0.1
    H = heads * d
    st = ops.DropoutState(dev)
    qkv = rnd(dev, N * T, 3 * H, seed=5).to(BF if bf else torch.float32).requires_grad_()
    mask = torch.zeros(N, T, device=dev)
    mask[0, T - 5:] = -10000.0
    bias = make_bias(dev, form, N, heads, T, T)[0].requires_grad_()
    dout = rnd(dev, N * T, H, seed=6).to(qkv.dtype)

    def step():
        out, _ = ops.SelfAttentionFn.apply(qkv, mask, N, T, heads, p, st.tensor, 9, bias)
        gq, gb = torch.autograd.grad(out, (qkv, bias), dout)
        return out.detach(), gq, gb

    eager = [t.clone() for t in step()]          # (st.tensor is this pass's frozen (seed, counter): eager and captured runs draw the same masks)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        captured = step()
    gr.replay()
    torch.cuda.synchronize()
    for a, b, what in zip(captured, eager, ("ctx", "dqkv", "dbias")):
        assert torch.equal(a, b), (what, float((a.float() - b.float()).abs().max()))
    assert float(captured[2].abs().max()) > 0


# ---- invariance ------------------------------------------------------------------------------------------------------------------------------
def _spy(fn, snap=None):
    """names (or snap(name, args), taken AT the call: the records the arguments point to die with the caller's frame) of every ops.call during fn()"""
    from ytvln import _lib, ops
    seen, real = [], _lib.call

    def spy(name, *a):
        seen.append(snap(name, a) if snap else name)
        return real(name, *a)

    _lib.call = ops.call = spy
    try:
        fn()
    finally:
        _lib.call = ops.call = real
    return seen


def test_default_and_constant_bias_steps_call_no_dbias_entry_point(dev, lib):
    from helpers import args_ns
    from ytvln import synth, utils_init
    from ytvln.optimization import AdamW
    from ytvln.vilbert_init import grouped_parameters
    args = args_ns(ranking=True, traj_judge=True, masked_vision=True, masked_language=True)
    batch = list(synth.to_torch(synth.make_batch(bs=2, K=7, T=16, frames=2, boxes=4, seed=9, ignore_rank_frac=0.0), dev))
    (bs, K, T), R = batch[6].shape[:3], batch[3].shape[2]
    batch[11] = torch.randint(-1, 2, (bs, K, R, T), generator=torch.Generator().manual_seed(3)).to(dev)          # co_attention_mask: one [R,T] mask per option
    for switch in (False, True):          # default step; step with the co-attention switch on and a constant (non-trainable) mask
        model, cfg = _lily(dev)
        model.train()
        next(m for m in model.modules() if type(m).__name__ == "BertModel").encoder.use_co_attention_mask = switch
        opt = AdamW(grouped_parameters(model, 0.01), lr=1e-3)
        names = _spy(lambda: utils_init.train_step(model, opt, None, batch, args, all_options=True))
        torch.cuda.synchronize()
        assert not [n for n in names if "dbias" in n]
        assert bool([n for n in names if "_bias_" in n]) == switch


@pytest.mark.parametrize("bf", [False, True])
def test_trainable_bias_launches_what_a_detached_one_launches(dev, lib, bf):
    """With a trainable bias the forward / backward entry points get the same arguments as with a detached one (same pointers, same records)
    and ctx / dq / dk / dv are bit-identical; the only difference is the dbias call behind the backward."""
    import ctypes
    from ytvln import _lib, ops
    N, T, heads, d = 2, 80, 4, 64
    H = heads * d
    qkv = rnd(dev, N * T, 3 * H, seed=5).to(BF if bf else torch.float32).requires_grad_()
    mask = torch.zeros(N, T, device=dev)
    bias = make_bias(dev, "n1", N, heads, T, T)[0]
    dout = rnd(dev, N * T, H, seed=6).to(qkv.dtype)
    st = ops.DropoutState(dev)          # (one frozen (seed, counter) record: both runs draw the same masks)
    runs = []
    for trainable in (False, True):
        b = bias.detach().requires_grad_(trainable)
        res = {}

        def go():
            out, lse = ops.SelfAttentionFn.apply(qkv, mask, N, T, heads, 0.1, st.tensor, 9, b)
            res["out"], res["lse"] = out.detach(), lse
            res["dqkv"], = torch.autograd.grad(out, (qkv,), dout, allow_unused=True)

        def key(name, a):          # a biased launch as (name, scalar arguments, the bias record's contents, the problem's read-only operands)
            if "_bias_" not in name:
                return (name,)
            rec, pr = _lib.AttnBias.from_address(a[1]), _lib.AttnProblem.from_address(a[0])
            return (name, a[4:8], (rec.ptr, rec.stride_n, rec.stride_h, rec.stride_q, rec.stride_k),
                    (pr.q, pr.k, pr.v, pr.mask, pr.ldq, pr.ldk, pr.ldv, pr.ldo, pr.Tq, pr.Tk, pr.p_drop, pr.site))

        calls = _spy(go, snap=key)
        runs.append((res, [c for c in calls if len(c) > 1], [c[0] for c in calls]))
        assert b.grad is None
    (r0, k0, n0), (r1, k1, n1) = runs
    assert k0 == k1 and len(k0) == 2
    assert n0 == [n for n in n1 if "dbias" not in n] and not [n for n in n0 if "dbias" in n]
    # (torch.autograd.grad for qkv alone: the bias gradient is not asked for, but the Function computes what needs_input_grad marked at forward time)
    assert [n for n in n1 if "dbias" in n] == ["ytvln_attn_dbias_bf16" if bf else "ytvln_attn_dbias_f32"]
    for k in ("out", "lse", "dqkv"):
        assert torch.equal(r0[k], r1[k]), k
