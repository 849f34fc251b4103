"""GPU: the per-score additive attention bias (ytvln_attn_bias: co_attention_mask and full 2-D masks) -- kernels against an fp64 restatement at
the bounds the unbiased tests of the same kernels use (tests/test_kernels_gpu.py: 2e-5 / 2e-5 forward, 2e-6 / 2e-5 probabilities, 2e-5 gradients;
tests/test_bf16_gpu.py: 1e-2 forward, 2e-2 gradients), every stride form, pair launches, "a zero bias changes nothing", full grids, the module
surface, the refusals that remain, and the guard that default runs never reach the new entry points."""
import math

import pytest
import torch

from helpers import close, rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def rnd(dev, *shape, seed=0, scale=0.5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev)


def make_bias(dev, form, N, heads, Tq, Tk, seed=7):
    """A bias in one of the accepted layouts; values: N(0,1) draws, 0 / +5 / -5 (a 0/+-1 co-attention mask times 5), -10000, and a few -inf
    placed so that key 0 of every query stays finite.  Returns (the tensor / view handed to the library, its dense [N, heads, Tq, Tk] fp64 value)."""
    g = torch.Generator().manual_seed(seed)
    shape = {"n1": (N, 1, Tq, Tk), "nh": (N, heads, Tq, Tk), "11": (1, 1, Tq, Tk), "n1T": (N, 1, Tk, Tq)}[form]
    b = torch.randn(shape, generator=g)
    u = torch.rand(shape, generator=g)
    b = torch.where(u < 0.15, torch.zeros(()), b)
    b = torch.where((u >= 0.15) & (u < 0.25), torch.full((), 5.0), b)
    b = torch.where((u >= 0.25) & (u < 0.35), torch.full((), -5.0), b)
    b = torch.where((u >= 0.35) & (u < 0.45), torch.full((), -10000.0), b)
    b = torch.where((u >= 0.45) & (u < 0.48), torch.full((), -float("inf")), b)
    if form == "n1T":
        b[:, :, 0, :] = torch.randn(b[:, :, 0, :].shape, generator=g)          # key 0 finite for every query
        t = b.to(dev)
        view = t.transpose(2, 3)
        assert not view.is_contiguous() or Tq == 1 or Tk == 1
        return view, view.double().expand(N, heads, Tq, Tk)
    b[:, :, :, 0] = torch.randn(b[:, :, :, 0].shape, generator=g)
    t = b.to(dev)
    return t, t.double().expand(N, heads, Tq, Tk)


def ref_attention(q, k, v, mask, bias, heads, keep=None, p=0.0):
    """fp64 restatement: q [N,Tq,H], k / v [N,Tk,H], mask [N,Tk] or None, bias dense [N,heads,Tq,Tk] or None -> ctx [N,Tq,H], probs"""
    N, Tq, H = q.shape
    d = H // heads
    qh, kh, vh = (t.view(N, -1, heads, d).permute(0, 2, 1, 3) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) / math.sqrt(d)
    if mask is not None:
        s = s + mask[:, None, None, :]
    if bias is not None:
        s = s + bias
    pr = torch.softmax(s, -1)
    pd = pr if keep is None else pr * keep / (1 - p)
    return (pd @ vh).permute(0, 2, 1, 3).reshape(N, Tq, H), pr


@pytest.fixture
def two_wave():
    """The fp32 kernel form biased problems use, pinned for the unbiased launches they are compared with bit for bit: no one-wave kernels, no
    d-split forward workgroups (the d-split form sums q.k in another order)."""
    from ytvln import _lib
    prev = (_lib.set_option("ATTN_W1", 0), _lib.set_option("ATTN_DSPLIT", 0))
    yield
    _lib.set_option("ATTN_W1", prev[0])
    _lib.set_option("ATTN_DSPLIT", prev[1])


# (N, heads, d, Tq, Tk): the cfg-2 co-attention pair in both directions, text self-attention, image self-attention at 288 / 576 / 808 regions
# (576 and 808 exceed the one-wave kernels' 512), T 60, ragged sizes, a padded head dimension
_SHAPES = [(2, 8, 128, 80, 288), (2, 8, 128, 288, 80), (2, 12, 64, 80, 80), (2, 8, 128, 288, 288), (1, 8, 128, 576, 576), (1, 8, 128, 808, 808),
           (2, 12, 64, 60, 60), (2, 8, 128, 33, 95), (2, 2, 64, 1, 95), (1, 3, 32, 33, 65), (2, 4, 8, 6, 5)]
_FORMS = ["n1", "nh", "11", "n1T"]


def _run_case(dev, N, heads, d, Tq, Tk, form, bf, with_mask=True):
    from ytvln import ops
    H = heads * d
    A = rnd(dev, N * Tq, 3 * H, seed=1)
    B = rnd(dev, N * Tk, 3 * H, seed=2)
    dout = rnd(dev, N * Tq, H, seed=3)
    if bf:
        A, B, dout = A.to(BF), B.to(BF), dout.to(BF)
    mask = None
    if with_mask:
        mask = torch.zeros(N, Tk, device=dev)
        mask[0, Tk - max(1, Tk // 4):] = -10000.0          # padded tail (key 0 stays open unless Tk == 1)
    bias, dense = make_bias(dev, form, N, heads, Tq, Tk)
    out = torch.empty(N * Tq, H, device=dev, dtype=A.dtype)
    scale = 1 / math.sqrt(d)
    lse = ops._attn_fwd(A, 0, 3 * H, B, H, 3 * H, B, 2 * H, 3 * H, mask, out, N, heads, Tq, Tk, d, scale, 0.0, None, 0, bias=bias)
    qd = A[:, :H].double().view(N, Tq, H).requires_grad_(True)
    kd = B[:, H:2 * H].double().reshape(N, Tk, H).requires_grad_(True)
    vd = B[:, 2 * H:].double().reshape(N, Tk, H).requires_grad_(True)
    ref, pr = ref_attention(qd, kd, vd, None if mask is None else mask.double(), dense, heads)
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(lse).all())
    probs = ops.attn_probs(A, 0, 3 * H, B, H, 3 * H, mask, lse, N, heads, Tq, Tk, d, scale, bias=bias)
    ref.backward(dout.double().view(N, Tq, H))
    gA, gB = torch.zeros_like(A), torch.zeros_like(B)
    ops._attn_bwd(A, 0, 3 * H, B, H, 3 * H, B, 2 * H, 3 * H, mask, out, dout, lse, gA, 0, 3 * H, gB, H, 3 * H, gB, 2 * H, 3 * H,
                  N, heads, Tq, Tk, d, scale, 0.0, None, 0, bias=bias)
    got = (gA[:, :H].reshape(N, Tq, H), gB[:, H:2 * H].reshape(N, Tk, H), gB[:, 2 * H:].reshape(N, Tk, H))
    errs = dict(fwd=rel_l2(out.view(N, Tq, H), ref), dq=rel_l2(got[0], qd.grad), dk=rel_l2(got[1], kd.grad), dv=rel_l2(got[2], vd.grad),
                probs=float((probs.double() - pr.detach()).abs().max()))
    print(f"attn bias {'bf16' if bf else 'fp32'} N{N} h{heads} d{d} Tq{Tq} Tk{Tk} {form}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    if bf:
        assert errs["fwd"] < 1e-2
        # probabilities: the kernel widens the bf16 projections and works in fp32 on the bf16 forward's log-sum-exp, whose error bound in
        # tests/test_bf16_gpu.py is 1e-2 absolute; p = exp(s - lse) <= 1, so |dp| <= p (e^{|d lse|} - 1) <= 1.01e-2
        assert errs["probs"] < 1.01e-2, errs
        assert errs["dq"] < 2e-2 and errs["dk"] < 2e-2 and errs["dv"] < 2e-2, errs
    else:
        close(out.view(N, Tq, H), ref, 2e-5, 2e-5, "attn fwd")
        close(probs, pr, 2e-6, 2e-5, "attn probs")
        assert errs["dq"] < 2e-5 and errs["dk"] < 2e-5 and errs["dv"] < 2e-5, errs
    assert float(gA[:, H:].float().abs().max()) == 0 and float(gB[:, :H].float().abs().max()) == 0, "only the addressed column blocks are written"


@pytest.mark.parametrize("form", _FORMS)
@pytest.mark.parametrize("N,heads,d,Tq,Tk", _SHAPES)
def test_attention_bias_fp32(dev, lib, N, heads, d, Tq, Tk, form):
    _run_case(dev, N, heads, d, Tq, Tk, form, bf=False)


@pytest.mark.parametrize("form", _FORMS)
@pytest.mark.parametrize("N,heads,d,Tq,Tk", [s for s in _SHAPES if s[2] in (64, 128)])
def test_attention_bias_bf16(dev, lib, N, heads, d, Tq, Tk, form):
    _run_case(dev, N, heads, d, Tq, Tk, form, bf=True)


def test_attention_bias_without_key_mask(dev, lib):
    """mask = NULL (what a full 2-D self-attention mask sends): + 0, exact."""
    _run_case(dev, 2, 12, 64, 80, 80, "nh", bf=False, with_mask=False)
    _run_case(dev, 2, 8, 128, 95, 95, "n1", bf=True, with_mask=False)


def _co_apply(dev, bf, p, biases, seed=11, N=2, R=72, T=20, heads=2, d=64, st=None):
    from ytvln import ops
    Hb = heads * d
    dt = BF if bf else torch.float32
    q1, kv1, q2, kv2 = (rnd(dev, N * n_, w * Hb, seed=seed + i).to(dt).requires_grad_() for i, (n_, w) in enumerate(((R, 1), (R, 2), (T, 1), (T, 2))))
    m1, m2 = torch.zeros(N, R, device=dev), torch.zeros(N, T, device=dev)
    m1[1, R - 9:] = -10000.0
    m2[0, T - 5:] = -10000.0
    args = (q1, kv1, q2, kv2, m1, m2, N, R, T, heads, p, p, st.tensor if st else None, 3, 4)
    c1, c2, l1, l2 = ops.CoAttentionFn.apply(*args, *(() if biases is None else biases))
    g1, g2 = rnd(dev, N * T, Hb, seed=91).to(dt), rnd(dev, N * R, Hb, seed=92).to(dt)
    torch.autograd.backward([c1, c2], [g1, g2])
    return [c1.detach(), c2.detach(), l1, l2] + [t.grad for t in (q1, kv1, q2, kv2)], (q1, kv1, q2, kv2, m1, m2, g1, g2)


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("sides", ["both", "first", "second", "neither"])
def test_pair_launch_with_bias_on_either_side(dev, lib, bf, sides):
    """Both directions of BertBiAttention in one launch, each with its own bias or none, against fp64; the co-attention mask's two readings
    ([N,1,R,T] as it lies for regions over tokens, its transposed VIEW for tokens over regions) are the forms used."""
    N, R, T, heads, d = 2, 72, 20, 2, 64
    co, dense2 = make_bias(dev, "n1", N, heads, R, T, seed=21)
    b1, b2 = co.transpose(2, 3), co
    biases = {"both": (b1, b2), "first": (b1, None), "second": (None, b2), "neither": None}[sides]
    got, (q1, kv1, q2, kv2, m1, m2, g1, g2) = _co_apply(dev, bf, 0.0, biases, N=N, R=R, T=T, heads=heads, d=d)
    Hb = heads * d
    dq1, dkv1, dq2, dkv2 = (t.detach().double().requires_grad_() for t in (q1, kv1, q2, kv2))
    d1 = dense2.transpose(2, 3) if sides in ("both", "first") else None
    d2 = dense2 if sides in ("both", "second") else None
    r1, _ = ref_attention(dq2.view(N, T, Hb), dkv1[:, :Hb].reshape(N, R, Hb), dkv1[:, Hb:].reshape(N, R, Hb), m1.double(), d1, heads)
    r2, _ = ref_attention(dq1.view(N, R, Hb), dkv2[:, :Hb].reshape(N, T, Hb), dkv2[:, Hb:].reshape(N, T, Hb), m2.double(), d2, heads)
    torch.autograd.backward([r1, r2], [g1.double().view(N, T, Hb), g2.double().view(N, R, Hb)])
    fb, gb = (1e-2, 2e-2) if bf else (2e-5, 2e-5)
    assert rel_l2(got[0].view(N, T, Hb), r1) < fb and rel_l2(got[1].view(N, R, Hb), r2) < fb
    for g_, r_, nme in zip(got[4:], (dq1, dkv1, dq2, dkv2), ("q1", "kv1", "q2", "kv2")):
        assert rel_l2(g_, r_.grad) < gb, (nme, rel_l2(g_, r_.grad))


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_zero_bias_changes_nothing(dev, lib, two_wave, bf, p):
    """On the kernel form biased problems use, an all-zero bias is the same launch bit for bit -- forward, log-sum-exp and backward, and with
    dropout the same keep decisions (fadd(x, 0) is exact; nothing else of the arithmetic depends on the flag)."""
    from ytvln import ops
    N, R, T, heads, d = 2, 288, 80, 4, 128
    st = ops.DropoutState(dev) if p > 0 else None
    z = torch.zeros(N, 1, R, T, device=dev)
    a, _ = _co_apply(dev, bf, p, None, N=N, R=R, T=T, heads=heads, d=d, st=st)
    b, _ = _co_apply(dev, bf, p, (z.transpose(2, 3), z), N=N, R=R, T=T, heads=heads, d=d, st=st)
    for x, y, nme in zip(a, b, ("ctx1", "ctx2", "lse1", "lse2", "dq1", "dkv1", "dq2", "dkv2")):
        assert torch.equal(x, y), (nme, float((x.float() - y.float()).abs().max()))
    # self-attention, d = 64, one problem
    H, T2 = 12 * 64, 80
    outs = []
    for bias in (None, torch.zeros(1, 1, T2, T2, device=dev)):
        qkv = rnd(dev, N * T2, 3 * H, seed=5).to(BF if bf else torch.float32).requires_grad_()
        mask = torch.zeros(N, T2, device=dev)
        mask[0, 70:] = -10000.0
        o, lse = ops.SelfAttentionFn.apply(qkv, mask, N, T2, 12, p, st.tensor if st else None, 9, *(() if bias is None else (bias,)))
        o.backward(rnd(dev, N * T2, H, seed=6).to(o.dtype))
        outs.append((o.detach(), lse, qkv.grad))
    for x, y in zip(*outs):
        assert torch.equal(x, y)


@pytest.mark.parametrize("precision,N,T,heads,d", [("bf16", 56, 288, 8, 128), ("bf16", 24, 576, 8, 128), ("fp32", 56, 80, 12, 64),
                                                    ("fp32", 56, 288, 8, 128)])
def test_attention_bias_full_grids_every_block_right_and_reproducible(dev, lib, precision, N, T, heads, d):
    """tests/test_bf16_gpu.py::test_attention_full_grids_every_block_right_and_reproducible with a bias (cfg-2 and cfg-5 attention sizes):
    every 32-query block against an fp32 softmax on the same inputs, four runs bit-identical, two of them while a second stream keeps the chip busy."""
    from ytvln import ops
    bf = precision == "bf16"
    g = torch.Generator().manual_seed(N + T + d)
    H = heads * d
    qkv = (torch.randn((N * T, 3 * H), generator=g) * 0.5).to(dev)
    qkv = (qkv.to(BF) if bf else qkv).requires_grad_()
    do = (torch.randn((N * T, H), generator=g) * 0.5).to(dev)
    do = do.to(BF) if bf else do
    mask = torch.zeros(N, T, device=dev)
    mask[:, T - 3:] = -10000.0
    bias = torch.randn((N, 1, T, T), generator=g).to(dev)
    frame = torch.arange(T, device=dev) // 36
    bias = bias + torch.where(frame[:, None] == frame[None, :], 0.0, -10000.0)          # block-diagonal "same frame" structure on top
    q, k, v = [qkv.detach()[:, j * H:(j + 1) * H].float().view(N, T, heads, d).transpose(1, 2) for j in range(3)]
    s = (q @ k.transpose(-1, -2)) / math.sqrt(d) + mask[:, None, None, :] + bias
    ref = torch.softmax(s, -1) @ v
    ref_lse = torch.logsumexp(s, -1)
    bar = 3e-2 if bf else 2e-5
    side = torch.cuda.Stream()
    A, B = torch.randn(4096, 1024, device=dev), torch.randn(1024, 1024, device=dev)
    runs = []
    for i in range(4):
        junk = torch.full((N * T, H), 7.0, device=dev, dtype=qkv.dtype)
        del junk                                                             # the kernel's output buffer starts as 7.0, not as the last result
        torch.cuda.synchronize()
        if i >= 2:
            with torch.cuda.stream(side):
                for _ in range(4):
                    ops.linear(A, B, None)
        qkv.grad = None
        out, lse = ops.SelfAttentionFn.apply(qkv, mask, N, T, heads, 0.0, None, 0, bias)
        out.backward(do)
        torch.cuda.synchronize()
        o = out.detach().float().view(N, T, heads, d).transpose(1, 2)
        err = (o - ref).abs().amax(-1)
        worst = float(err.max())
        assert worst < bar, (i, worst, (err > bar).nonzero()[:8].tolist())
        assert float((lse - ref_lse).abs().max()) < (1e-2 if bf else 1e-4)
        runs.append((out.detach().clone(), lse.detach().clone(), qkv.grad.clone()))
    for i in range(1, 4):
        for a, b, what in zip(runs[i], runs[0], ("out", "lse", "dqkv")):
            assert torch.equal(a, b), (i, what, float((a.float() - b.float()).abs().max()))


# ---- module surface -----------------------------------------------------------------------------------------------------------------------
def _micro_cfg(**over):
    from helpers import ZERO_DROP, cfg_dict
    from ytvln.vilbert import BertConfig
    d = cfg_dict("tiny_2_2_1.json", **ZERO_DROP)
    d.update(over)
    return BertConfig(**d)


def test_self_attention_modules_take_full_masks_and_refuse_the_rest(dev, lib):
    """BertSelfAttention / BertImageSelfAttention with [N,1,T,T] (causal), [N,h,T,T] and [1,1,T,T] masks against the fp64 restatement of
    vilbert.py:284-311 on the module's own weights, at the fp32 bars of DESIGN.md section 2 (1e-4 + 1e-4 |ref| on outputs and probabilities,
    gradient rel-L2 <= 1e-4); other shapes still raise, and so does a bias that requires grad."""
    from ytvln import ops
    from ytvln.vilbert import BertImageSelfAttention, BertSelfAttention
    cfg = _micro_cfg()
    torch.manual_seed(0)
    for cls, hidden, heads in ((BertSelfAttention, cfg.hidden_size, cfg.num_attention_heads),
                               (BertImageSelfAttention, cfg.v_hidden_size, cfg.v_num_attention_heads)):
        m = cls(cfg).to(dev).eval()
        m.want_probs = True
        N, T = 3, 9
        causal = torch.where(torch.ones(T, T).tril().bool(), 0.0, -10000.0).to(dev)
        for mask in (causal.expand(N, 1, T, T), causal[None, None], (causal + torch.randn(N, heads, T, T, device=dev)),
                     causal[None, None].expand(N, 1, T, T).contiguous()):
            x = rnd(dev, N, T, hidden, seed=3).requires_grad_()
            out, probs = m(x, mask)
            gy = rnd(dev, N, T, hidden, seed=4)
            m.zero_grad()
            out.backward(gy)
            xd = x.detach().double().requires_grad_()
            W = {k: v.detach().double().requires_grad_() for k, v in m.named_parameters()}
            q, k, v = (xd @ W[f"{n}.weight"].t() + W[f"{n}.bias"] for n in ("query", "key", "value"))
            ref, pr = ref_attention(q, k, v, None, mask.double().expand(N, heads, T, T), heads)
            ref.backward(gy.double())
            close(out, ref, 1e-4, 1e-4, "context")
            close(probs, pr, 1e-4, 1e-4, "probs")
            assert rel_l2(x.grad, xd.grad) < 1e-4
            for n_, p_ in m.named_parameters():
                if n_ == "key.bias":
                    # a shift common to all keys of a row cancels in the softmax: this gradient is exactly zero, and a relative error against
                    # zero means nothing -- it is held to the same 1e-4, relative to the query bias' gradient (same units, same sums)
                    assert float(p_.grad.double().norm()) < 1e-4 * float(W["query.bias"].grad.norm()), n_
                    continue
                assert rel_l2(p_.grad, W[n_].grad) < 1e-4, n_
        x = rnd(dev, N, T, hidden, seed=3)
        for bad in (torch.zeros(N, 1, T, T + 1, device=dev), torch.zeros(N, T, T, device=dev), torch.zeros(2, 1, T, T, device=dev)):
            with pytest.raises(NotImplementedError, match="accepted are"):
                m(x, bad)
        with pytest.raises(RuntimeError, match="requires_grad"):
            m(x, torch.zeros(N, 1, T, T, device=dev, requires_grad=True))
        # a per-key mask keeps today's path: no bias entry point is reached
        calls = _count_bias_calls(lambda: m(x, torch.zeros(N, 1, 1, T, device=dev)))
        assert calls == 0


def _count_bias_calls(fn):
    from ytvln import _lib, ops
    seen, real = [], _lib.call

    def spy(name, *a):
        if "_bias_" in name:
            seen.append(name)
        return real(name, *a)

    _lib.call = ops.call = spy          # (ops binds the name at import)
    try:
        fn()
    finally:
        _lib.call = ops.call = real
    return len(seen)


def _ref_connection(layer, x1, m1, x2, m2, co, heads):
    """fp64 restatement of BertBiAttention with use_co_attention_mask=True (vilbert.py:552-618) on the layer's own weights."""
    W = {k: v.detach().double() for k, v in layer.named_parameters()}
    lin = lambda x, n: x @ W[f"{n}.weight"].t() + W[f"{n}.bias"]          # noqa: E731
    q1, k1, v1 = (lin(x1, f"biattention.{n}1") for n in ("query", "key", "value"))
    q2, k2, v2 = (lin(x2, f"biattention.{n}2") for n in ("query", "key", "value"))
    N, R, T = x1.shape[0], x1.shape[1], x2.shape[1]
    c1, p1 = ref_attention(q2, k1, v1, m1.reshape(N, R), co.transpose(2, 3).expand(N, heads, T, R), heads)
    c2, p2 = ref_attention(q1, k2, v2, m2.reshape(N, T), co.expand(N, heads, R, T), heads)
    return c1, c2, p1, p2


@pytest.mark.parametrize("R,T", [(5, 6), (70, 45)])
def test_biattention_with_co_attention_mask(dev, lib, R, T):
    """BertBiAttention.forward(..., co_attention_mask, use_co_attention_mask=True): both contexts and both probability tensors against the
    fp64 restatement, key masks with padding on both sides at once; the switch off ignores the argument bit for bit."""
    from ytvln.vilbert import BertConnectionLayer
    cfg = _micro_cfg()
    torch.manual_seed(1)
    layer = BertConnectionLayer(cfg).to(dev).eval()
    layer.biattention.want_probs = True
    N, heads = 6, cfg.bi_num_attention_heads
    x1, x2 = rnd(dev, N, R, cfg.v_hidden_size, seed=1), rnd(dev, N, T, cfg.hidden_size, seed=2)
    m1, m2 = torch.zeros(N, 1, 1, R, device=dev), torch.zeros(N, 1, 1, T, device=dev)
    m1[0, ..., R - 2:] = -10000.0
    m2[0, ..., T - 3:] = -10000.0
    m2[1, ..., T - 1:] = -10000.0
    co, _ = make_bias(dev, "n1", N, heads, R, T, seed=5)
    c1, c2, (p1, p2) = layer.biattention(x1, m1, x2, m2, co, True)
    r1, r2, q1, q2 = _ref_connection(layer, x1.double(), m1.double(), x2.double(), m2.double(), co.double(), heads)
    close(c1, r1, 1e-4, 1e-4, "context 1")
    close(c2, r2, 1e-4, 1e-4, "context 2")
    close(p1, q1, 1e-4, 1e-4, "probs 1")
    close(p2, q2, 1e-4, 1e-4, "probs 2")
    off = layer.biattention(x1, m1, x2, m2, co, False)
    none = layer.biattention(x1, m1, x2, m2, None, False)
    assert torch.equal(off[0], none[0]) and torch.equal(off[1], none[1])
    assert not torch.equal(off[0], c1)
    o1, o2, _ = layer(x1, m1, x2, m2, co, True)          # the whole connection layer runs, backward included
    (o1.sum() + o2.sum()).backward()
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in layer.parameters())
    with pytest.raises(NotImplementedError, match="co_attention_mask of shape"):
        layer.biattention(x1, m1, x2, m2, torch.zeros(N, 1, T, R + 1, device=dev), True)


def _lily(dev, seed=3, **over):
    from helpers import args_ns
    from ytvln import synth
    from ytvln.lily import Lily
    cfg = _micro_cfg(**over)
    cfg.args = args_ns(ranking=True, traj_judge=True, masked_vision=True, masked_language=True)
    model = Lily(cfg, dropout_prob=0.0)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    W = synth.make_weights(shapes, seed=seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    return model.to(dev), cfg


def _bert_inputs(dev, N=4, T=7, R=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 50, (N, T), generator=g).to(dev)
    feats = torch.randn((N, R, 2048), generator=g).to(dev)
    loc = torch.rand((N, R, 12), generator=g).to(dev)          # (5 box + 4 orientation + 2 next-orientation + frame)
    am = torch.ones(N, T)
    am[0, T - 2:] = 0
    vm = torch.ones(N, R)
    vm[1, R - 1:] = 0
    co = (torch.randint(-1, 2, (N, R, T), generator=g)).float().to(dev)
    return ids, feats, loc, am.to(dev), vm.to(dev), co


@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
def test_model_switch_off_ignores_the_mask_and_on_uses_it(dev, lib, precision):
    """BertModel: flag off (the default, the reference's :736) with a non-zero co_attention_mask equals the run with None bit for bit and
    reaches no bias entry point; flag on changes the outputs, equals the run whose mask is zero only when the mask IS zero, and two-stream on
    equals off bit for bit."""
    from ytvln import ops
    model, cfg = _lily(dev)
    bert = next(m for m in model.modules() if type(m).__name__ == "BertModel").eval()
    ids, feats, loc, am, vm, co = _bert_inputs(dev, R=5)
    prev = ops.get_matmul_precision()
    ops.set_matmul_precision(precision)
    try:
        run = lambda c: bert(ids, feats, loc, None, am, vm, c)[:2]          # noqa: E731
        with torch.no_grad():
            assert bert.encoder.use_co_attention_mask is False
            a, b = run(co), run(None)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            assert _count_bias_calls(lambda: run(co)) == 0
            bert.encoder.use_co_attention_mask = True
            try:
                on = run(co)
                assert _count_bias_calls(lambda: run(co)) > 0
                assert not torch.equal(on[0], a[0])
                zero = run(torch.zeros_like(co))
                close(zero[0], a[0], 1e-4, 1e-4, "zero mask, switch on, against switch off (other kernel form: to rounding)")
                tsp = ops.get_two_stream()
                ops.set_two_stream(not tsp)
                try:
                    other = run(co)
                finally:
                    ops.set_two_stream(tsp)
                assert torch.equal(other[0], on[0]) and torch.equal(other[1], on[1]), "two-stream on == off, bit for bit"
            finally:
                bert.encoder.use_co_attention_mask = False
    finally:
        ops.set_matmul_precision(prev)


def test_default_training_step_calls_no_bias_entry_point(dev, lib):
    """Guard: a default training step (no co-attention switch, per-key masks) launches exactly what it launched before -- none of the
    ytvln_attn_*_bias_* entry points is called."""
    from helpers import args_ns
    from ytvln import synth, utils_init
    from ytvln.optimization import AdamW
    from ytvln.vilbert_init import grouped_parameters
    model, cfg = _lily(dev)
    model.train()
    args = args_ns(ranking=True, traj_judge=True, masked_vision=True, masked_language=True)
    batch = synth.to_torch(synth.make_batch(bs=2, K=7, T=16, frames=2, boxes=4, seed=9, ignore_rank_frac=0.0), dev)
    opt = AdamW(grouped_parameters(model, 0.01), lr=1e-3)
    n = _count_bias_calls(lambda: utils_init.train_step(model, opt, None, batch, args, all_options=True))
    torch.cuda.synchronize()
    assert n == 0
