"""Parity of every C-ABI kernel with a plain fp64/fp32 torch restatement of the same op (GPU box only)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import close, gold, rel_l2

pytestmark = pytest.mark.gpu


def rnd(dev, *shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


# ------------------------------------------------------------------------------------------------------------------
# GEMM
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(130, 70, 50), (256, 256, 64), (64, 64, 32), (4480, 768, 768), (57, 1001, 64), (300, 12, 11),
                                   (1024, 3072, 768), (33, 1, 256), (2016, 1024, 2048)])
def test_gemm_layouts(dev, lib, M, N, K):
    from ytvln import ops
    A = rnd(dev, M, K, seed=1)
    Bt = rnd(dev, N, K, seed=2)          # nn.Linear layout [N, K]
    bias = rnd(dev, N, seed=3)
    ref = (A.double() @ Bt.double().t() + bias.double())
    # NT (forward)
    C = torch.empty(M, N, device=dev)
    ops._gemm(A, K, 0, Bt, K, 1, C, N, M, N, K, bias=bias)
    close(C, ref, 2e-4 * math.sqrt(K / 64), 1e-4, "NT")
    # NN: dX = dY[M,N] . W[N,K]
    dY = rnd(dev, M, N, seed=4)
    dX = torch.empty(M, K, device=dev)
    ops._gemm(dY, N, 0, Bt, K, 0, dX, K, M, K, N)
    close(dX, dY.double() @ Bt.double(), 2e-4 * math.sqrt(N / 64) + 1e-5, 1e-4, "NN")
    # TN: dW = dY^T . A  -> [N, K]
    dW = torch.empty(N, K, device=dev)
    ops._gemm(dY, N, 1, A, K, 0, dW, K, N, K, M)
    close(dW, dY.double().t() @ A.double(), 2e-4 * math.sqrt(M / 64) + 1e-5, 1e-4, "TN")
    # transpose detection: asymmetric check of one element
    i, j = M // 3, N // 2
    assert abs(float(C[i, j]) - float(ref[i, j])) < 1e-2


def test_gemm_epilogues_and_strides(dev, lib):
    from ytvln import ops
    from ytvln._lib import EPI_GELU, EPI_MUL_DGELU, EPI_MUL_DRELU, EPI_RELU
    M, N, K = 200, 136, 96
    A, W, b = rnd(dev, M, K, seed=1), rnd(dev, N, K, seed=2), rnd(dev, N, seed=3)
    z = A.double() @ W.double().t() + b.double()
    C, aux = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)
    ops._gemm(A, K, 0, W, K, 1, C, N, M, N, K, bias=b, aux=aux, ldaux=N, epi=EPI_GELU)
    close(aux, z, 2e-4, 1e-4, "gelu pre-activation")
    close(C, F.gelu(z), 2e-4, 1e-4, "gelu")
    ops._gemm(A, K, 0, W, K, 1, C, N, M, N, K, bias=b, epi=EPI_RELU)
    close(C, z.clamp(min=0), 2e-4, 1e-4, "relu")
    # MUL_DGELU: C = (A.B) * gelu'(aux)
    zz = rnd(dev, M, N, seed=5)
    zd = zz.double().requires_grad_(True)
    F.gelu(zd).sum().backward()
    ops._gemm(A, K, 0, W, K, 1, C, N, M, N, K, aux=zz, ldaux=N, epi=EPI_MUL_DGELU)
    close(C, (A.double() @ W.double().t()) * zd.grad, 3e-4, 2e-4, "mul_dgelu")
    ops._gemm(A, K, 0, W, K, 1, C, N, M, N, K, aux=zz, ldaux=N, epi=EPI_MUL_DRELU)
    close(C, (A.double() @ W.double().t()) * (zz > 0).double(), 3e-4, 2e-4, "mul_drelu")
    # beta = 1 accumulates
    C0 = rnd(dev, M, N, seed=6)
    C1 = C0.clone()
    ops._gemm(A, K, 0, W, K, 1, C1, N, M, N, K, beta=1.0)
    close(C1, C0.double() + A.double() @ W.double().t(), 3e-4, 1e-4, "beta=1")
    # strided A (first-token pooling: lda = T*H) and padded C (ldc > N)
    T = 5
    X = rnd(dev, M, T, K, seed=7)
    Cp = torch.zeros(M, N + 8, device=dev)
    ops._gemm(X, T * K, 0, W, K, 1, Cp, N + 8, M, N, K, bias=b)
    close(Cp[:, :N], X[:, 0].double() @ W.double().t() + b.double(), 2e-4, 1e-4, "strided")
    assert float(Cp[:, N:].abs().max()) == 0.0
    # unaligned leading dimensions (scalar-load path): lda = K+1
    Au = torch.zeros(M, K + 1, device=dev)
    Au[:, :K] = A
    ops._gemm(Au, K + 1, 0, W, K, 1, C, N, M, N, K)
    close(C, A.double() @ W.double().t(), 2e-4, 1e-4, "unaligned lda")


def test_linear_and_ffn_autograd(dev, lib):
    from ytvln import ops
    M, K, I, N = 150, 64, 96, 48
    x, w1, b1 = rnd(dev, 3, M // 3, K, seed=1), rnd(dev, I, K, seed=2, scale=0.2), rnd(dev, I, seed=3)
    w2, b2 = rnd(dev, N, I, seed=4, scale=0.2), rnd(dev, N, seed=5)
    ts = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    y = ops.ffn(*ts)
    g = rnd(dev, *y.shape, seed=9)
    y.backward(g)
    td = [t.detach().double().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    yr = F.linear(F.gelu(F.linear(td[0], td[1], td[2])), td[3], td[4])
    yr.backward(g.double())
    close(y, yr, 3e-4, 2e-4, "ffn fwd")
    for a, b_, nme in zip(ts, td, "x w1 b1 w2 b2".split()):
        assert rel_l2(a.grad, b_.grad) < 2e-5, nme
    # plain linear with relu
    ts = [t.clone().requires_grad_(True) for t in (x, w1, b1)]
    y = ops.linear(ts[0], ts[1], ts[2], "relu")
    g = rnd(dev, *y.shape, seed=10)
    y.backward(g)
    td = [t.detach().double().requires_grad_(True) for t in (x, w1, b1)]
    yr = F.relu(F.linear(*td))
    yr.backward(g.double())
    close(y, yr, 3e-4, 2e-4, "linear relu")
    for a, b_, nme in zip(ts, td, "x w b".split()):
        assert rel_l2(a.grad, b_.grad) < 2e-5, nme


# ------------------------------------------------------------------------------------------------------------------
# reductions / scatters
# ------------------------------------------------------------------------------------------------------------------
def test_colsum_variants(dev, lib):
    from ytvln import ops
    for M, N in [(1000, 70), (4480, 768), (5, 30522), (1, 3)]:
        x = rnd(dev, M, N, seed=M)
        close(ops.colsum(x, M, N, N), x.double().sum(0), 1e-3, 1e-5, f"colsum {M}x{N}")
    M, N, KT = 3001, 130, 32
    x = rnd(dev, M, N, seed=3)
    idx = torch.randint(0, KT, (M,), generator=torch.Generator().manual_seed(1)).to(dev)
    ref = torch.zeros(KT, N, dtype=torch.float64, device=dev).index_add_(0, idx, x.double())
    close(ops.colsum_by_index(x, M, N, N, KT, idx_i64=idx), ref, 1e-3, 1e-5, "by index i64")
    loc = torch.zeros(M, 12, device=dev)
    loc[:, 11] = idx.float()
    close(ops.colsum_by_index(x, M, N, N, KT, idx_f32=loc, idx_stride=12, idx_f32_offset=11), ref, 1e-3, 1e-5, "by index f32")
    tg = torch.zeros(97, N, device=dev)
    ids = torch.randint(0, 97, (M,), generator=torch.Generator().manual_seed(2)).to(dev)
    from ytvln._lib import call
    call("ytvln_scatter_add_rows_f32", x.data_ptr(), N, ids.data_ptr(), M, N, tg.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    ref = torch.zeros(97, N, dtype=torch.float64, device=dev).index_add_(0, ids, x.double())
    ref[0] = 0
    close(tg, ref, 1e-3, 1e-5, "scatter_add_rows with padding_idx")


# ------------------------------------------------------------------------------------------------------------------
# LayerNorm family
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,H", [(7, 32), (50, 48), (33, 256), (4480, 768), (2016, 1024), (5, 2048)])
def test_layernorm_fwd_bwd(dev, lib, rows, H):
    from ytvln import ops
    import vilbert_ref as O
    x, r = rnd(dev, rows, H, seed=1), rnd(dev, rows, H, seed=2)
    g, b = 1 + 0.1 * rnd(dev, H, seed=3), 0.1 * rnd(dev, H, seed=4)
    ts = [t.clone().requires_grad_(True) for t in (x, r, g, b)]
    y = ops.add_layer_norm(ts[0], ts[1], ts[2], ts[3])
    dy = rnd(dev, rows, H, seed=5)
    y.backward(dy)
    td = [t.detach().double().requires_grad_(True) for t in (x, r, g, b)]
    yr = O.layer_norm(td[0] + td[1], td[2], td[3])
    yr.backward(dy.double())
    close(y, yr, 2e-5, 2e-5, "ln fwd")
    for a, b_, nme in zip(ts, td, "x res gamma beta".split()):
        assert rel_l2(a.grad, b_.grad) < 1e-5, nme
    # no residual, constant row (variance 0 -> eps inside sqrt)
    xc = x.clone()
    xc[0] = 2.5
    close(ops.add_layer_norm(xc, None, g, b), O.layer_norm(xc.double(), g.double(), b.double()), 2e-5, 2e-5, "ln const row")


def test_layernorm_kat_from_reference(dev, lib):
    from ytvln import ops
    k = gold("g5_kats.npz")
    y = ops.add_layer_norm(torch.from_numpy(k["ln/x"]).to(dev), None, torch.from_numpy(k["ln/w"]).to(dev), torch.from_numpy(k["ln/b"]).to(dev))
    close(y, k["ln/y"], 1e-5, 1e-5, "reference BertLayerNorm KAT")


def test_dropout_masks_consistent(dev, lib):
    from ytvln import ops
    st = ops.DropoutState(dev)
    n = 1 << 20
    x = torch.ones(n + 3, device=dev, requires_grad=True)
    y = ops.dropout(x, 0.1, True, st)
    keep = (y != 0).float()
    assert abs(float(keep.mean()) - 0.9) < 3e-3
    close(y[y != 0], torch.full_like(y[y != 0], 1 / 0.9), 1e-6, 1e-6)
    y.backward(torch.ones_like(y))
    assert torch.equal(x.grad, y.detach()), "backward must regenerate the forward mask"
    # different sites / different forwards give different masks
    y2 = ops.dropout(x.detach(), 0.1, True, st)
    assert float(((y2 != 0) != (y != 0)).float().mean()) > 0.1
    st2 = ops.DropoutState(dev)
    st2._site = 0
    y3 = ops.dropout(x.detach(), 0.1, True, st2)
    assert float(((y3 != 0) != (y != 0)).float().mean()) > 0.1
    # LN with pre / post dropout: gradient consistency through the recomputed masks
    rows, H = 64, 256
    xx, rr = rnd(dev, rows, H, seed=1), rnd(dev, rows, H, seed=2)
    g, b = 1 + 0.1 * rnd(dev, H, seed=3), 0.1 * rnd(dev, H, seed=4)
    for p_pre, p_post in ((0.25, 0.0), (0.0, 0.25)):
        st = ops.DropoutState(dev)
        ts = [t.clone().requires_grad_(True) for t in (xx, rr, g, b)]
        y = ops.add_layer_norm(ts[0], ts[1], ts[2], ts[3], 1e-12, p_pre, p_post, st)
        dy = rnd(dev, rows, H, seed=5)
        y.backward(dy)
        # recover the masks with probe inputs through the same site
        st_probe = ops.DropoutState.__new__(ops.DropoutState)
        st_probe.tensor, st_probe._site = st.tensor, 0
        probe = ops.DropoutFn.apply(torch.ones(rows, H, device=dev), max(p_pre, p_post), st.tensor, 1)
        td = [t.detach().double().requires_grad_(True) for t in (xx, rr, g, b)]
        import vilbert_ref as O
        if p_pre > 0:
            yr = O.layer_norm(td[0] * probe.double() + td[1], td[2], td[3])
        else:
            yr = O.layer_norm(td[0] + td[1], td[2], td[3]) * probe.double()
        yr.backward(dy.double())
        close(y, yr, 3e-5, 3e-5, f"ln dropout fwd {p_pre},{p_post}")
        for a, b_, nme in zip(ts, td, "x res gamma beta".split()):
            assert rel_l2(a.grad, b_.grad) < 1e-5, (nme, p_pre, p_post)


def test_embeddings(dev, lib):
    from ytvln import ops
    import vilbert_ref as O
    N, T, H, V = 6, 9, 48, 97
    S = {"e.word_embeddings.weight": rnd(dev, V, H, seed=1), "e.position_embeddings.weight": rnd(dev, 32, H, seed=2),
         "e.token_type_embeddings.weight": rnd(dev, 2, H, seed=3), "e.LayerNorm.weight": 1 + 0.1 * rnd(dev, H, seed=4),
         "e.LayerNorm.bias": 0.1 * rnd(dev, H, seed=5)}
    ids = torch.randint(0, V, (N, T), generator=torch.Generator().manual_seed(1)).to(dev)
    ids[0, :3] = 0
    tt = torch.randint(0, 2, (N, T), generator=torch.Generator().manual_seed(2)).to(dev)
    names = list(S)
    ts = [S[k].clone().requires_grad_(True) for k in names]
    y = ops.text_embed(ids, tt, *ts)
    dy = rnd(dev, N, T, H, seed=7)
    y.backward(dy)
    Sd = {k: v.detach().double().requires_grad_(True) for k, v in S.items()}
    # nn.Embedding(padding_idx=0) semantics: row 0 is used in forward but receives no gradient
    yr = O.text_embeddings(Sd, ids, tt, pre="e.")
    yr.backward(dy.double())
    close(y, yr, 2e-5, 2e-5, "text embed fwd")
    refg = Sd["e.word_embeddings.weight"].grad.clone()
    refg[0] = 0
    assert rel_l2(ts[0].grad, refg) < 1e-5
    for i in range(1, 5):
        assert rel_l2(ts[i].grad, Sd[names[i]].grad) < 1e-5, names[i]
    # token_type_ids=None path
    close(ops.text_embed(ids, None, *[S[k] for k in names]), O.text_embeddings({k: v.double() for k, v in S.items()}, ids, None, pre="e."), 2e-5, 2e-5)

    # image embeddings
    R, Fdim, Hv = 10, 16, 64
    P = {"v.image_embeddings.weight": rnd(dev, Hv, Fdim, seed=11, scale=0.3), "v.image_embeddings.bias": rnd(dev, Hv, seed=12),
         "v.image_location_embeddings.weight": rnd(dev, Hv, 5, seed=13), "v.image_location_embeddings.bias": rnd(dev, Hv, seed=14),
         "v.image_orientation_embeddings.weight": rnd(dev, Hv, 4, seed=15), "v.image_orientation_embeddings.bias": rnd(dev, Hv, seed=16),
         "v.image_next_orientation_embeddings.weight": rnd(dev, Hv, 2, seed=17), "v.image_next_orientation_embeddings.bias": rnd(dev, Hv, seed=18),
         "v.image_sequence_embeddings.weight": rnd(dev, 32, Hv, seed=19), "v.LayerNorm.weight": 1 + 0.1 * rnd(dev, Hv, seed=20),
         "v.LayerNorm.bias": 0.1 * rnd(dev, Hv, seed=21)}
    feat = rnd(dev, N, R, Fdim, seed=30).clamp(min=0)
    loc = rnd(dev, N, R, 12, seed=31)
    loc[..., 11] = torch.randint(0, 8, (N, R), generator=torch.Generator().manual_seed(3)).float().to(dev)
    pn = list(P)
    ps = [P[k].clone().requires_grad_(True) for k in pn]
    img = ops.linear(feat, ps[0], ps[1])
    y = ops.image_embed(img, loc, ps[2], ps[3], ps[4], ps[5], ps[6], ps[7], ps[8], ps[9], ps[10])
    dy = rnd(dev, N, R, Hv, seed=33)
    y.backward(dy)
    Pd = {k: v.detach().double().requires_grad_(True) for k, v in P.items()}
    yr = O.image_embeddings(Pd, feat.double(), loc.double(), pre="v.")
    yr.backward(dy.double())
    close(y, yr, 3e-5, 3e-5, "image embed fwd")
    for i, k in enumerate(pn):
        assert rel_l2(ps[i].grad, Pd[k].grad) < 2e-5, k


# ------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------
def ref_attention(q, k, v, mask, heads, dropmask=None, p=0.0):
    """q [N,Tq,H], k/v [N,Tk,H] (double), mask additive [N,Tk] -> ctx [N,Tq,H], probs"""
    N, Tq, H = q.shape
    d = H // heads
    qh, kh, vh = (t.view(N, -1, heads, d).permute(0, 2, 1, 3) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) / math.sqrt(d) + mask[:, None, None, :]
    pr = torch.softmax(s, -1)
    pd = pr if dropmask is None else pr * dropmask / (1 - p)
    return (pd @ vh).permute(0, 2, 1, 3).reshape(N, Tq, H), pr


@pytest.fixture
def attn_form(request):
    """Selects the attention kernel forms through the library's run-time options (include/ytvln.h: ytvln_set_option) for one test:
    "default" = what a training step takes; "w1_dkv" = the one-wave-per-SIMD dK/dV kernel forced for launches of ANY size (by default it is
    only taken when its last round of wave slots is >= 85 % full, i.e. never at the small shapes below -- VERDICT r3 item 4);
    "two_wave" = the round-2 two-wave / wave-pair kernels everywhere."""
    from ytvln import _lib
    form = getattr(request, "param", "default")
    prev = {}
    if form == "w1_dkv":
        prev["ATTN_W1_DKV_ANY"] = _lib.set_option("ATTN_W1_DKV_ANY", 1)
    elif form == "two_wave":
        prev["ATTN_W1"] = _lib.set_option("ATTN_W1", 0)
    yield form
    for k, v in prev.items():
        _lib.set_option(k, v)


_ATTN_SHAPES = [(2, 4, 8, 8, 6), (2, 4, 12, 6, 6), (3, 4, 64, 80, 80), (2, 8, 128, 288, 288), (2, 8, 128, 80, 288), (2, 8, 128, 288, 80),
                (2, 2, 64, 16, 8), (1, 2, 128, 252, 100), (1, 3, 32, 33, 65), (1, 2, 64, 1000, 808), (1, 1, 128, 1, 3), (1, 2, 64, 512, 512),
                # query / key counts around the 32-row granule of the text stream (T = 80) and of short instructions
                (2, 8, 128, 17, 95), (2, 8, 128, 95, 17), (2, 8, 128, 16, 80), (2, 8, 128, 80, 16), (2, 12, 64, 17, 16), (2, 12, 64, 95, 80)]
# the one-wave dK/dV kernel directly against fp64: unpadded d = 128 / d = 64 heads, ragged query / key tiles, fully masked rows, 576 keys,
# single tile; (29, 8, 128, 288, 288) has 2088 wave slots >= 2 rounds of 1024 and takes that kernel by the DEFAULT selection
_W1_SHAPES = [(3, 4, 64, 80, 80), (2, 8, 128, 288, 288), (2, 8, 128, 80, 288), (2, 8, 128, 288, 80), (2, 2, 64, 16, 8), (1, 2, 128, 252, 100),
              (2, 2, 128, 37, 101), (1, 1, 128, 1, 3), (1, 2, 64, 512, 512), (1, 2, 128, 100, 576), (2, 3, 64, 33, 288),
              (2, 8, 128, 17, 95), (2, 8, 128, 95, 17), (2, 8, 128, 16, 80), (2, 8, 128, 80, 16), (2, 12, 64, 17, 16), (2, 12, 64, 95, 80)]


@pytest.mark.parametrize("N,heads,d,Tq,Tk,attn_form",
                         [s + ("default",) for s in _ATTN_SHAPES] + [s + ("w1_dkv",) for s in _W1_SHAPES] +
                         [(29, 8, 128, 288, 288, "default"), (3, 4, 64, 80, 80, "two_wave"), (2, 8, 128, 288, 288, "two_wave")],
                         indirect=["attn_form"])
def test_attention_fwd_bwd(dev, lib, N, heads, d, Tq, Tk, attn_form):
    from ytvln import ops
    H = heads * d
    # packed projections with 3H columns, as produced by the fused QKV GEMM
    A = rnd(dev, N * Tq, 3 * H, seed=1)
    B = rnd(dev, N * Tk, 3 * H, seed=2)
    mask = torch.zeros(N, Tk, device=dev)
    mask[0, Tk - max(1, Tk // 4):] = -10000.0          # padded tail
    if N > 1:
        mask[1, :] = -10000.0                          # fully masked row (softmax over equal shifts)
    out = torch.empty(N * Tq, H, device=dev)
    scale = 1 / math.sqrt(d)
    lse = ops._attn_fwd(A, 0, 3 * H, B, H, 3 * H, B, 2 * H, 3 * H, mask, out, N, heads, Tq, Tk, d, scale, 0.0, None, 0)
    qd = A[:, :H].double().view(N, Tq, H).requires_grad_(True)
    kd = B[:, H:2 * H].double().reshape(N, Tk, H).requires_grad_(True)
    vd = B[:, 2 * H:].double().reshape(N, Tk, H).requires_grad_(True)
    ref, pr = ref_attention(qd, kd, vd, mask.double(), heads)
    # rows whose keys are ALL masked add -10000 to every score: fp32 then quantises scores to ~1e-3 (as the reference's
    # own fp32 arithmetic does), so those rows are compared with an fp32 restatement at a matching tolerance.
    full = [n for n in range(N) if bool((mask[n] != 0).all())]
    part = [n for n in range(N) if n not in full]
    close(out.view(N, Tq, H)[part], ref[part], 2e-5, 2e-5, "attn fwd")
    probs = ops.attn_probs(A, 0, 3 * H, B, H, 3 * H, mask, lse, N, heads, Tq, Tk, d, scale)
    close(probs[part], pr[part], 2e-6, 2e-5, "attn probs")
    if full:
        r32, p32 = ref_attention(qd.float(), kd.float(), vd.float(), mask, heads)
        close(out.view(N, Tq, H)[full], r32[full], 5e-3, 5e-3, "attn fwd (fully masked rows, fp32 yardstick)")
        close(probs[full], p32[full], 5e-3, 5e-3, "attn probs (fully masked rows)")
    dout = rnd(dev, N * Tq, H, seed=3)
    ref.backward(dout.double().view(N, Tq, H))
    gA, gB = torch.zeros_like(A), torch.zeros_like(B)
    ops._attn_bwd(A, 0, 3 * H, B, H, 3 * H, B, 2 * H, 3 * H, mask, out, dout, lse, gA, 0, 3 * H, gB, H, 3 * H, gB, 2 * H, 3 * H,
                  N, heads, Tq, Tk, d, scale, 0.0, None, 0)
    tol = lambda rows: 2e-5 if rows is part else 5e-3     # noqa: E731
    for rows in (part, full):
        if rows:
            assert rel_l2(gA[:, :H].reshape(N, Tq, H)[rows], qd.grad[rows]) < tol(rows), "dq"
            assert rel_l2(gB[:, H:2 * H].reshape(N, Tk, H)[rows], kd.grad[rows]) < tol(rows), "dk"
            assert rel_l2(gB[:, 2 * H:].reshape(N, Tk, H)[rows], vd.grad[rows]) < tol(rows), "dv"
    assert float(gA[:, H:].abs().max()) == 0 and float(gB[:, :H].abs().max()) == 0, "only the addressed column blocks are written"


def test_attention_softmax_kat(dev, lib):
    """masked softmax KAT produced by torch.softmax in the reference process (fully masked tail + fully masked row)."""
    from ytvln import ops
    k = gold("g5_kats.npz")
    s, m, p = (torch.from_numpy(k[f"softmax/{n}"]) for n in ("s", "mask", "p"))
    # realise the scores s as q.k with d = Tk one-hot keys: q_i = s_i * sqrt(d) padded, k_j = e_j
    N, h, Tq, Tk = s.shape
    d = 12
    kk = torch.zeros(N, Tk, h, d)
    for j in range(Tk):
        kk[:, j, :, j] = 1.0
    # reference computed softmax(s / sqrt(8) + mask); our kernel computes q.k / sqrt(d): fold both scalings into q
    q = torch.zeros(N, Tq, h, d)
    q[..., :Tk] = s.permute(0, 2, 1, 3) * (math.sqrt(d) / math.sqrt(8))
    add = ((1.0 - m) * -10000.0).to(dev)
    qf, kf = q.reshape(N * Tq, h * d).to(dev), kk.reshape(N * Tk, h * d).to(dev)
    out = torch.empty(N * Tq, h * d, device=dev)
    lse = ops._attn_fwd(qf, 0, h * d, kf, 0, h * d, kf, 0, h * d, add, out, N, h, Tq, Tk, d, 1 / math.sqrt(d), 0.0, None, 0)
    probs = ops.attn_probs(qf, 0, h * d, kf, 0, h * d, add, lse, N, h, Tq, Tk, d, 1 / math.sqrt(d))
    close(probs[0], p[0], 2e-6, 2e-5, "masked softmax KAT (masked tail)")
    close(probs[1], p[1], 5e-3, 5e-3, "masked softmax KAT (fully masked row: fp32 score quantisation at -10000)")


@pytest.mark.parametrize("d,attn_form", [(128, "default"), (128, "w1_dkv"), (64, "w1_dkv"), (128, "two_wave")], indirect=["attn_form"])
def test_attention_dropout(dev, lib, d, attn_form):
    from ytvln import ops
    N, heads, Tq, p = 2, 2, 40, 0.2
    Tk = 96 if d >= 96 else 64          # (the mask-recovery trick below needs Tk <= d)
    H = heads * d
    st = ops.DropoutState(dev)
    site = 5
    scale = 1 / math.sqrt(d)
    # recover the keep mask: q = k = 0 -> uniform probs; v = identity columns -> out[i, j] = keep_ij / (Tk (1-p))
    z = torch.zeros(N * Tq, H, device=dev)
    zk = torch.zeros(N * Tk, H, device=dev)
    eye = torch.zeros(N, Tk, heads, d, device=dev)
    for j in range(Tk):
        eye[:, j, :, j] = 1.0
    eye = eye.reshape(N * Tk, H)
    out = torch.empty(N * Tq, H, device=dev)
    ops._attn_fwd(z, 0, H, zk, 0, H, eye, 0, H, None, out, N, heads, Tq, Tk, d, scale, p, st.tensor, site)
    keep = (out.view(N, Tq, heads, d)[..., :Tk] > 0).permute(0, 2, 1, 3).double()      # [N,h,Tq,Tk]
    assert abs(float(keep.mean()) - (1 - p)) < 0.02
    q, k, v = rnd(dev, N * Tq, H, seed=1), rnd(dev, N * Tk, H, seed=2), rnd(dev, N * Tk, H, seed=3)
    mask = torch.zeros(N, Tk, device=dev)
    mask[0, Tk * 5 // 6:] = -10000.0
    lse = ops._attn_fwd(q, 0, H, k, 0, H, v, 0, H, mask, out, N, heads, Tq, Tk, d, scale, p, st.tensor, site)
    qd, kd, vd = (t.double().view(N, -1, H).requires_grad_(True) for t in (q, k, v))
    ref, _ = ref_attention(qd, kd, vd, mask.double(), heads, keep, p)
    close(out.view(N, Tq, H), ref, 3e-5, 3e-5, "attn dropout fwd")
    dout = rnd(dev, N * Tq, H, seed=4)
    ref.backward(dout.double().view(N, Tq, H))
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    ops._attn_bwd(q, 0, H, k, 0, H, v, 0, H, mask, out, dout, lse, dq, 0, H, dk, 0, H, dv, 0, H, N, heads, Tq, Tk, d, scale, p,
                  st.tensor, site)
    assert rel_l2(dq.view(N, Tq, H), qd.grad) < 3e-5
    assert rel_l2(dk.view(N, Tk, H), kd.grad) < 3e-5
    assert rel_l2(dv.view(N, Tk, H), vd.grad) < 3e-5


def test_self_and_co_attention_functions(dev, lib):
    from ytvln import ops
    N, R, T, heads, d = 2, 40, 12, 4, 32
    Hb = heads * d
    q1 = rnd(dev, N * R, Hb, seed=1).requires_grad_(True)
    kv1 = rnd(dev, N * R, 2 * Hb, seed=2).requires_grad_(True)
    q2 = rnd(dev, N * T, Hb, seed=3).requires_grad_(True)
    kv2 = rnd(dev, N * T, 2 * Hb, seed=4).requires_grad_(True)
    m1, m2 = torch.zeros(N, R, device=dev), torch.zeros(N, T, device=dev)
    m1[1, 30:] = -10000.0
    m2[0, 9:] = -10000.0
    c1, c2, _, _ = ops.CoAttentionFn.apply(q1, kv1, q2, kv2, m1, m2, N, R, T, heads, 0.0, 0.0, None, 0, 0)
    g1, g2 = rnd(dev, *c1.shape, seed=5), rnd(dev, *c2.shape, seed=6)
    (c1 * g1).sum().add((c2 * g2).sum()).backward()
    a1, b1, a2, b2 = (t.detach().double().requires_grad_(True) for t in (q1, kv1, q2, kv2))
    r1, _ = ref_attention(a2.view(N, T, Hb), b1[:, :Hb].reshape(N, R, Hb), b1[:, Hb:].reshape(N, R, Hb), m1.double(), heads)
    r2, _ = ref_attention(a1.view(N, R, Hb), b2[:, :Hb].reshape(N, T, Hb), b2[:, Hb:].reshape(N, T, Hb), m2.double(), heads)
    ((r1.reshape(N * T, Hb) * g1.double()).sum() + (r2.reshape(N * R, Hb) * g2.double()).sum()).backward()
    close(c1, r1.reshape(N * T, Hb), 2e-5, 2e-5, "ctx1")
    close(c2, r2.reshape(N * R, Hb), 2e-5, 2e-5, "ctx2")
    for got, ref, nme in ((q1, a1, "q1"), (kv1, b1, "kv1"), (q2, a2, "q2"), (kv2, b2, "kv2")):
        assert rel_l2(got.grad, ref.grad) < 2e-5, nme
    # a dead direction must propagate None (reference autograd semantics; AdamW skips grad-None tensors)
    for t in (q1, kv1, q2, kv2):
        t.grad = None
    c1, c2, _, _ = ops.CoAttentionFn.apply(q1, kv1, q2, kv2, m1, m2, N, R, T, heads, 0.0, 0.0, None, 0, 0)
    (c1 * g1).sum().backward()
    assert q1.grad is None and kv2.grad is None and q2.grad is not None and kv1.grad is not None


# ------------------------------------------------------------------------------------------------------------------
# losses and optimizer
# ------------------------------------------------------------------------------------------------------------------
def test_losses(dev, lib):
    from ytvln import ops
    k = gold("g5_kats.npz")
    lg, tg = torch.from_numpy(k["ce/logits"]).to(dev).requires_grad_(True), torch.from_numpy(k["ce/target"]).to(dev)
    l = ops.cross_entropy(lg, tg, -1)
    close(l, k["ce/loss"], 1e-6, 1e-6, "ce KAT")
    l.backward()
    ld = lg.detach().double().requires_grad_(True)
    F.cross_entropy(ld, tg, ignore_index=-1).backward()
    assert rel_l2(lg.grad, ld.grad) < 1e-6
    assert math.isnan(float(ops.cross_entropy(lg.detach(), torch.full((6,), -1, device=dev), -1))) and math.isnan(float(k["ce/all_ignored"]))
    close(ops.cross_entropy(torch.from_numpy(k["ce/logits_inf"]).to(dev), torch.from_numpy(k["ce/target_inf"]).to(dev), -1), k["ce/loss_inf"], 1e-6, 1e-6, "ce -inf KAT")
    # large vocabulary, padded leading dimension
    M, V = 300, 30522
    big = rnd(dev, M, V + 6, seed=1)[:, :V]
    t = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(1)).to(dev)
    t[::3] = -1
    bigr = big.clone().requires_grad_(True)
    l = ops.cross_entropy(bigr, t, -1)
    bd = big.double().requires_grad_(True)
    lr_ = F.cross_entropy(bd, t, ignore_index=-1)
    close(l, lr_, 2e-6, 2e-6, "ce big")
    (l * 3.0).backward()
    (lr_ * 3.0).backward()
    assert rel_l2(bigr.grad, bd.grad) < 1e-5
    # KL
    pr, tt = torch.from_numpy(k["kl/pred"]).to(dev), torch.from_numpy(k["kl/target"]).to(dev)
    for nm in ("some", "none"):
        mk = torch.from_numpy(k[f"kl/{nm}_mask"]).to(dev)
        prr = pr.clone().requires_grad_(True)
        l = ops.kl_masked(prr, tt, mk)
        close(l, k[f"kl/{nm}_loss"], 1e-6, 1e-6, f"kl KAT {nm}")
        l.backward()
        pd = pr.double().requires_grad_(True)
        lr_ = (F.kl_div(F.log_softmax(pd, -1), tt.double(), reduction="none") * mk.unsqueeze(-1).double()).sum() / max(1, int(mk.sum()))
        lr_.backward()
        close(prr.grad, pd.grad, 1e-7, 1e-5, f"kl grad {nm}")
    M, C = 500, 1601
    pr = rnd(dev, M, C, seed=2)
    tt = torch.softmax(rnd(dev, M, C, seed=3) * 3, -1)
    mk = (torch.rand(M, generator=torch.Generator().manual_seed(4)) < 0.15).long().to(dev)
    prr = pr.clone().requires_grad_(True)
    l = ops.kl_masked(prr, tt, mk)
    pd = pr.double().requires_grad_(True)
    lr_ = (F.kl_div(F.log_softmax(pd, -1), tt.double(), reduction="none") * mk.unsqueeze(-1).double()).sum() / max(1, int(mk.sum()))
    close(l, lr_, 2e-6, 2e-6, "kl big")
    l.backward(); lr_.backward()
    assert rel_l2(prr.grad, pd.grad) < 1e-5
    # BCE
    x, t, pw = (torch.from_numpy(k[f"bce/{n}"]).to(dev) for n in ("logits", "target", "pos_weight"))
    xr = x.clone().requires_grad_(True)
    l = ops.bce_with_logits(xr, t, pw)
    close(l, k["bce/loss"], 1e-6, 1e-6, "bce KAT")
    l.backward()
    xd = x.double().requires_grad_(True)
    F.binary_cross_entropy_with_logits(xd, t.double(), pos_weight=pw.double()).backward()
    assert rel_l2(xr.grad, xd.grad) < 1e-6
    close(ops.bce_with_logits(x, t), F.binary_cross_entropy_with_logits(x.double(), t.double()), 1e-6, 1e-6, "bce no pos_weight")


def test_gelu_kat_and_act_bwd(dev, lib):
    from ytvln import ops
    from ytvln._lib import EPI_GELU
    k = gold("g5_kats.npz")
    x = torch.from_numpy(k["gelu/x"]).to(dev)
    n = x.numel()
    eye = torch.eye(n, device=dev)
    y = ops.linear(x.view(1, n), eye, None, "gelu")
    close(y.view(-1), k["gelu/y"], 1e-6, 1e-6, "reference gelu KAT")


def test_adamw_kernel_matches_reference_kat(dev, lib):
    from ytvln.optimization import AdamW
    k = gold("g5_kats.npz")
    p = torch.nn.Parameter(torch.from_numpy(k["adamw/p0"].copy()).to(dev))
    opt = AdamW([{"params": [p], "weight_decay": 0.01}], lr=1e-2)
    for i in range(3):
        p.grad = torch.from_numpy(k["adamw/grads"][i].copy()).to(dev)
        opt.step()
        close(p, k[f"adamw/p{i + 1}"], 1e-6, 2e-6, f"adamw step {i + 1}")
    close(opt.state[p]["exp_avg"], k["adamw/m"], 1e-8, 2e-6, "exp_avg")
    close(opt.state[p]["exp_avg_sq"], k["adamw/v"], 1e-9, 2e-5, "exp_avg_sq")
    assert opt.state[p]["step"] == 3


def test_gemm_zero_padded_tails(dev, lib):
    """Fast-path GEMM with a zero-padded K tail (K % 32 != 0, B rows clamped) and an M tail (M % 4 != 0) -- the shapes of
    the 30522-wide logit gradient (dX = dlogits . E, dE = dlogits^T . h)."""
    from ytvln import ops
    from ytvln._lib import GEMM_A_ZERO_PADDED
    M, V, H = 300, 1001 + 32 * 3 + 5, 96         # V = 1102: not a multiple of 4 or 32
    ld = (V + 31) // 32 * 32
    dl = torch.zeros(M, ld, device=dev)
    dl[:, :V] = rnd(dev, M, V, seed=1)
    E, h = rnd(dev, V, H, seed=2), rnd(dev, M, H, seed=3)
    dx = torch.empty(M, H, device=dev)
    ops._gemm(dl, ld, 0, E, H, 0, dx, H, M, H, V, flags=GEMM_A_ZERO_PADDED)          # K = V with a tail
    close(dx, dl[:, :V].double() @ E.double(), 1e-3, 1e-4, "dX with K tail")
    dE = torch.empty(V, H, device=dev)
    ops._gemm(dl, ld, 1, h, H, 0, dE, H, V, H, M, flags=GEMM_A_ZERO_PADDED)          # M = V with a tail
    close(dE, dl[:, :V].double().t() @ h.double(), 1e-3, 1e-4, "dW with M tail")
    # the same through autograd: linear -> cross-entropy with a wide odd vocabulary keeps the padded leading dimension
    x = rnd(dev, M, H, seed=4).requires_grad_(True)
    W = (rnd(dev, 1601, H, seed=5) * 0.1).requires_grad_(True)
    b = rnd(dev, 1601, seed=6).requires_grad_(True)
    t = torch.randint(0, 1601, (M,), generator=torch.Generator().manual_seed(1)).to(dev)
    logits = ops.linear(x, W, b)
    assert logits.shape == (M, 1601) and logits.stride(0) == 1632
    ops.cross_entropy(logits, t, -1).backward()
    xd, Wd, bd = (v.detach().double().requires_grad_(True) for v in (x, W, b))
    F.cross_entropy(F.linear(xd, Wd, bd), t).backward()
    for a, r, nme in ((x, xd, "x"), (W, Wd, "W"), (b, bd, "b")):
        assert rel_l2(a.grad, r.grad) < 2e-5, nme


def test_gemm_decoder_input_gradient_full_size_on_the_long_k_plan(dev, lib):
    """dX of the 30522-wide LM decoder at its cfg-2 size (vilbert.py:906 backward): 4480 x 768 x 30522 with A's K tail zero padded.  Since round 6
    the planner gives this launch ONE round of 160x256 tiles with three splits (tests/test_abi.py pins the plan); every 128x128 block of the
    result against fp64, and the launch is bit-reproducible."""
    import ctypes
    from ytvln import ops, _lib
    from ytvln._lib import GEMM_A_ZERO_PADDED
    M, V, H = 4480, 30522, 768
    tm, tn, sp = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert _lib.load().ytvln_gemm_plan(M, H, (V + 31) // 32 * 32, 0, 0, ctypes.byref(tm), ctypes.byref(tn), ctypes.byref(sp)) == 0
    assert (tm.value, tn.value, sp.value) == (160, 256, 3)
    ld = (V + 31) // 32 * 32
    dl = torch.zeros(M, ld, device=dev)
    dl[:, :V] = rnd(dev, M, V, seed=1) * 0.1
    E = rnd(dev, V, H, seed=2)
    ref = dl[:, :V].double() @ E.double()
    dx = torch.empty(M, H, device=dev)
    ops._gemm(dl, ld, 0, E, H, 0, dx, H, M, H, V, flags=GEMM_A_ZERO_PADDED)
    err = (dx.double() - ref).abs()
    blocks = err.view(M // 128, 128, H // 128, 128).amax(dim=(1, 3))          # (the bar of tests/test_gemm_sk_gpu.py for the same product)
    assert float(blocks.max()) < 4e-6 * math.sqrt(V) + 1e-6, float(blocks.max())
    dx2 = torch.empty(M, H, device=dev)
    ops._gemm(dl, ld, 0, E, H, 0, dx2, H, M, H, V, flags=GEMM_A_ZERO_PADDED)
    assert torch.equal(dx, dx2)


@pytest.mark.parametrize("M,N,K,ta,tb,epi", [
    (384, 256, 256, 0, 1, 0), (300, 200, 96, 0, 0, 0), (300, 200, 96, 1, 0, 0), (260, 132, 64, 1, 1, 0), (512, 384, 256, 0, 1, 1),
    (128, 256, 4096, 1, 0, 0), (1000, 520, 160, 0, 1, 3),
    (3600, 3592, 128, 0, 1, 0), (4096, 1024, 512, 0, 0, 0), (3080, 1024, 96, 0, 1, 1),      # 256-row tiles
    (1024, 1024, 4096, 1, 0, 0), (772, 3072, 1024, 1, 0, 0)])      # weight-gradient layout (M-contiguous A) on 256x256 tiles with split-K
def test_gemm_fp32_split_bf16x3(dev, lib, M, N, K, ta, tb, epi):
    """fp32x3 projections (YTVLN_GEMM_SPLIT_BF16X3): fp32 operands, every value split exactly into three bf16 terms in registers,
    six bf16 MFMAs per product with fp32 accumulation.  Bar: the SAME as the native fp32 MFMA path -- max error against the fp64
    product within 4e-6 * sqrt(K) * |a||b| scale -- and no worse than 2x the native kernel's own error on the same inputs; the
    result must differ from the native kernel's somewhere (it really is a different instruction stream, no silent fallback)."""
    from ytvln import ops
    g = torch.Generator().manual_seed(M + 3 * N + 7 * K)
    A = torch.randn((K, M) if ta else (M, K), generator=g).to(dev)
    B = torch.randn((N, K) if tb else (K, N), generator=g).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    aux_in = torch.randn(M, N, generator=g).to(dev)
    outs = {}
    for mode in ("fp32", "fp32x3"):
        C = torch.empty(M, N, device=dev)
        aux = aux_in.clone() if epi == 3 else (torch.empty(M, N, device=dev) if epi else None)
        ops.set_matmul_precision(mode)
        try:
            ops._gemm(A, A.stride(0), ta, B, B.stride(0), tb, C, N, M, N, K, bias=None if epi == 3 else bias, aux=aux, ldaux=N, epi=epi)
        finally:
            ops.set_matmul_precision("fp32")
        outs[mode] = C.double().cpu()
    ref = (A.t() if ta else A).double().cpu() @ (B if tb else B.t()).double().cpu().t()
    if epi == 3:        # EPI_MUL_DGELU: C = product * gelu'(aux)
        z = aux_in.double().cpu()
        ref = ref * (0.5 * (1 + torch.erf(z / 2 ** 0.5)) + z * torch.exp(-0.5 * z * z) / (2 * torch.pi) ** 0.5)
    else:
        ref = ref + bias.double().cpu()
        if epi == 1:
            ref = torch.nn.functional.gelu(ref)
    e_native = float((outs["fp32"] - ref).abs().max())
    e_split = float((outs["fp32x3"] - ref).abs().max())
    tol = 4e-6 * (K ** 0.5) * 4.0 + 1e-5
    assert e_split < tol, (e_split, tol)
    assert e_split < 2.0 * e_native + 1e-6, (e_split, e_native)
    assert not torch.equal(outs["fp32"], outs["fp32x3"]), "fp32x3 reproduced the native kernel bit for bit: the split path did not run"


def test_gemm_fp32_split_bf16x3_dynamic_range(dev, lib):
    """The three-term split is exact for every finite fp32 value (bf16 shares fp32's exponent range), so rows / columns scaled over
    twenty orders of magnitude keep the fp32-level error RELATIVE to their own scale (a bf16-rounded operand would be off by 4e-3)."""
    from ytvln import ops
    g = torch.Generator().manual_seed(5)
    M, N, K = 512, 384, 256
    sa = 10.0 ** (torch.rand(M, 1, generator=g) * 20 - 10)
    sb = 10.0 ** (torch.rand(N, 1, generator=g) * 20 - 10)
    A = (torch.randn(M, K, generator=g) * sa).to(dev)
    B = (torch.randn(N, K, generator=g) * sb).to(dev)
    C = torch.empty(M, N, device=dev)
    ops.set_matmul_precision("fp32x3")
    try:
        ops._gemm(A, K, 0, B, K, 1, C, N, M, N, K)
    finally:
        ops.set_matmul_precision("fp32")
    ref = A.double().cpu() @ B.double().cpu().t()
    scale = (A.double().cpu().abs() @ B.double().cpu().abs().t())          # sum_k |a||b|: the natural error scale of a dot product
    rel = float(((C.double().cpu() - ref).abs() / scale).max())
    assert rel < 2e-6, rel


def test_gemm_fp32_split_bf16x3_adversarial_error_bound(dev, lib):
    """adversarial operands for the three-term form next to the native instruction, both against fp64, error measured in
    units of sum_k |a||b| (the forward error scale of a dot product; an fp32 accumulation of K terms is allowed ~K^0.5 .. K ulps of it):
      * catastrophic cancellation: every row of A is paired with columns built so that the exact dot product is ~1e-7 of sum |a||b|;
      * mixed signs over a long contraction (K = 8192) with magnitudes spread over 2^-20 .. 2^20 inside one dot product;
      * denormal-adjacent: operands at 2^-126 .. 2^-100 whose PRODUCTS are far below the fp32 range except against a large partner
        (the split terms mid / lo of such values are themselves subnormal or zero: the split must stay exact);
      * values with all 24 significand bits set (worst case for the hi / mid / lo split).
    The three-term result must stay within 4x the native kernel's own error bound on every case and must not be worse than 3x the native
    kernel's measured error (plus a small floor), i.e. it is an fp32-level arithmetic on these inputs too, not a reduced-precision mode."""
    from ytvln import ops
    g = torch.Generator().manual_seed(99)

    def run(A, B, mode):
        M, K = A.shape
        N = B.shape[0]
        C = torch.empty(M, N, device=dev)
        ops.set_matmul_precision(mode)
        try:
            ops._gemm(A.to(dev), K, 0, B.to(dev), K, 1, C, N, M, N, K)
        finally:
            ops.set_matmul_precision("fp32")
        return C.double().cpu()

    cases = {}
    M, N, K = 256, 256, 2048
    # cancellation: B's second half of the contraction is the negated first half plus a 1e-7 relative perturbation
    a = torch.randn(M, K // 2, generator=g)
    b = torch.randn(N, K // 2, generator=g)
    cases["cancellation"] = (torch.cat([a, a], 1), torch.cat([b, -b * (1 + 1e-7 * torch.randn(N, K // 2, generator=g))], 1))
    K2 = 8192
    mag = 2.0 ** torch.randint(-20, 21, (1, K2), generator=g).float()
    cases["mixed_sign_long_k"] = (torch.randn(M, K2, generator=g) * mag, torch.randn(N, K2, generator=g) / mag * torch.sign(torch.randn(N, K2, generator=g)))
    tiny = 2.0 ** torch.randint(-126, -99, (M, K), generator=g).float() * torch.sign(torch.randn(M, K, generator=g))
    huge = 2.0 ** torch.randint(90, 120, (N, K), generator=g).float() * (1 + torch.rand(N, K, generator=g))
    cases["denormal_adjacent"] = (tiny, huge)
    full = torch.full((M, K), float.fromhex("0x1.fffffep+0")) * torch.sign(torch.randn(M, K, generator=g))
    cases["all_significand_bits"] = (full, torch.full((N, K), float.fromhex("0x1.fffffep-1")) * (1 + 2.0 ** -23 * torch.randint(0, 2, (N, K), generator=g).float()))
    for name, (A, B) in cases.items():
        A, B = A.float().contiguous(), B.float().contiguous()
        assert torch.isfinite(A).all() and torch.isfinite(B).all()
        ref = A.double() @ B.double().t()
        scale = A.double().abs() @ B.double().abs().t()
        e_nat = float(((run(A, B, "fp32") - ref).abs() / scale).max())
        e_x3 = float(((run(A, B, "fp32x3") - ref).abs() / scale).max())
        kk = A.shape[1]
        bound = 6e-8 * (kk ** 0.5) * 4.0          # ~4 x (unit roundoff x sqrt(K)): the native kernel's own accumulation noise
        assert e_nat < bound, (name, "native", e_nat, bound)
        assert e_x3 < bound, (name, "fp32x3", e_x3, bound)
        assert e_x3 < 3.0 * e_nat + 2e-7, (name, e_x3, e_nat)


def test_edge_cases_and_loud_failures(dev, lib):
    """Empty problems are no-ops; illegal arguments raise with the library's message (no silent fallback of any kind)."""
    from ytvln import ops
    from ytvln._lib import call
    A = torch.randn(8, 16, device=dev)
    C = torch.full((4, 4), 7.0, device=dev)
    # M == 0 / N == 0: nothing is launched, C untouched
    call("ytvln_gemm_f32", A.data_ptr(), 16, 0, A.data_ptr(), 16, 1, C.data_ptr(), 4, None, None, 0, 0, 4, 16, 0, 0.0, None, 0, 0, None)
    assert float(C.min()) == 7.0
    with pytest.raises(RuntimeError, match="leading dimension"):
        call("ytvln_gemm_f32", A.data_ptr(), 8, 0, A.data_ptr(), 16, 1, C.data_ptr(), 4, None, None, 0, 4, 4, 16, 0, 0.0, None, 0, 0, None)
    with pytest.raises(RuntimeError, match="epilogue"):
        call("ytvln_gemm_f32", A.data_ptr(), 16, 0, A.data_ptr(), 16, 1, C.data_ptr(), 4, None, None, 0, 4, 4, 16, 9, 0.0, None, 0, 0, None)
    with pytest.raises(RuntimeError, match="head dim"):
        ops._attn_fwd(A, 0, 16, A, 0, 16, A, 0, 16, None, torch.empty(8, 16, device=dev), 1, 1, 8, 8, 6, 1.0, 0.0, None, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.linear(torch.randn(4, 16), torch.randn(8, 16, device=dev))
    with pytest.raises(RuntimeError, match="float32"):
        ops.linear(torch.randn(4, 16, device=dev, dtype=torch.float64), torch.randn(8, 16, device=dev))
    with pytest.raises(RuntimeError, match="output type"):          # the bf16-resident GEMM: C is bf16 or fp32, nothing else
        call("ytvln_gemm_bf16", A.data_ptr(), 16, 0, A.data_ptr(), 16, 1, C.data_ptr(), 8, 7, None, None, 0, 8, 8, 16, 0, 0.0, None, 0, 0, None, None, None)
    with pytest.raises(RuntimeError, match="head dim"):             # ... and its attention kernels exist for d = 64 / 128
        ops.SelfAttentionFn.apply(torch.zeros(8, 48, device=dev, dtype=torch.bfloat16), torch.zeros(1, 8, device=dev), 1, 8, 1, 0.0, None, 0)
    # empty row sets through the row kernels
    out = torch.empty(0, 16, device=dev)
    call("ytvln_gather_rows_f32", A.data_ptr(), 16, None, 0, 16, out.data_ptr(), None)
    assert ops.select_rows(torch.zeros(5, dtype=torch.bool, device=dev), 3).tolist() == [0, 1, 2]


def test_batch_masking_matches_reference_golden(dev, lib):
    """csrc/batch.hip with explicit draws == the reference's randomize_tokens / randomize_regions, bit for bit (integers and fp32
    copies / zeros), on the fixture generated by running the reference (tests/golden/g7_masking.npz)."""
    from helpers import gold
    from ytvln import batch as B
    g = gold("g7_masking.npz")
    t = lambda k: torch.from_numpy(g[k]).to(dev)   # noqa: E731
    tok, tgt = B.randomize_tokens(t("tokens"), t("mask"), p=t("p_tok"), random_tokens=t("rnd_tok"))
    assert torch.equal(tok, t("out_tok")) and torch.equal(tgt, t("tgt_tok"))
    feats = t("feats").clone()
    f, tg, m = B.randomize_regions(feats, t("probs"), t("rmask"), p=t("p_reg"))
    assert f.data_ptr() == feats.data_ptr()                      # in place, like the reference
    assert torch.equal(f, t("out_f")) and torch.equal(tg, t("out_t")) and torch.equal(m, t("out_m"))


def test_batch_masking_philox_statistics(dev, lib):
    """Production mode (Philox draws) at the BASELINE config-2 batch size: the masking rates of common.py:213-300 within 4 sigma,
    structural invariants exactly, a fresh mask on every call."""
    from ytvln import batch as B, synth
    nb = synth.make_batch(bs=8, K=7, T=80, frames=8, boxes=36, seed=3, ignore_rank_frac=0.0)
    bt = synth.to_torch(nb, dev)
    tokens, imask = bt[6].clone(), bt[7]
    orig = torch.where(bt[8] != -1, bt[8], tokens)               # undo the generator's own masking: start from clean tokens
    out, tgt = B.randomize_tokens(orig, imask)
    valid = imask.bool()
    sel = tgt != -1
    n = int(valid.sum())
    assert not bool(sel[~valid].any())                           # padding is never a target
    assert torch.equal(tgt[sel], orig[sel])                      # targets hold the original ids
    rate = float(sel.sum()) / n
    assert abs(rate - 0.15) < 4 * (0.15 * 0.85 / n) ** 0.5, rate
    frac_mask = float((out[sel] == 103).sum()) / int(sel.sum())
    frac_keep = float((out[sel] == orig[sel]).sum()) / int(sel.sum())
    ns = int(sel.sum())
    assert abs(frac_mask - 0.8) < 4 * (0.16 / ns) ** 0.5 and abs(frac_keep - 0.1) < 4 * (0.09 / ns) ** 0.5 + 1e-3, (frac_mask, frac_keep)
    assert torch.equal(out[~sel], orig[~sel])
    out2, tgt2 = B.randomize_tokens(orig, imask)
    assert not torch.equal(tgt, tgt2)                            # the device-side counter advanced
    feats = torch.relu(torch.randn(56, 288, 2048, device=dev))
    probs = torch.softmax(torch.randn(56, 288, 1601, device=dev), -1)
    keep = feats.clone()
    rmask = bt[3].reshape(56, 288)
    f, targets, tm = B.randomize_regions(feats, probs, rmask)
    rv = rmask.bool()
    assert not bool(tm[~rv].any())
    r = float(tm.sum()) / int(rv.sum())
    assert abs(r - 0.15) < 4 * (0.15 * 0.85 / int(rv.sum())) ** 0.5, r
    s = tm.bool()
    assert torch.equal(targets[s], probs[s]) and bool((targets[~s] == 1.0 / 1601).all())
    zeroed = (f.abs().sum(-1) == 0) & (keep.abs().sum(-1) != 0)
    assert not bool((zeroed & ~s).any())                         # only selected regions are zeroed
    zf = float(zeroed.sum()) / int(s.sum())
    assert abs(zf - 0.9) < 4 * (0.09 / int(s.sum())) ** 0.5, zf
    assert torch.equal(f[~zeroed], keep[~zeroed])


def test_expand_options_matches_host_expansion(dev, lib):
    """ytvln.batch.expand_options == materialising the K options on the host the way the reference's dataset does (positive path,
    shared-feature caption negatives, frame permutations, frames swapped for other photos, padded frames)."""
    from ytvln import batch as B
    g = torch.Generator().manual_seed(5)
    P, boxes, F, C, bs, K, frames = 23, 6, 64, 21, 3, 7, 4
    pf = torch.relu(torch.randn(P, boxes, F, generator=g))
    pb = torch.rand(P, boxes, 12, generator=g)
    pp = torch.softmax(torch.randn(P, boxes, C, generator=g), -1)
    pm = (torch.rand(P, boxes, generator=g) < 0.8).long()
    index = torch.full((bs, K, frames), -1, dtype=torch.int64)
    for b in range(bs):
        L = 2 + b % 3                                             # path length (the rest is padding)
        path = torch.randperm(P, generator=g)[:L]
        index[b, 0, :L] = index[b, 1, :L] = index[b, 2, :L] = path            # positive + two caption negatives share the frames
        index[b, 3, :L] = path[torch.randperm(L, generator=g)]                  # frame permutations
        index[b, 4, :L] = path[torch.randperm(L, generator=g)]
        for k in (5, 6):                                                        # some frames swapped for random photos
            alt = path.clone()
            alt[int(torch.randint(0, L, (1,), generator=g))] = int(torch.randint(0, P, (1,), generator=g))
            index[b, k, :L] = alt
    f, bx, pr, m = B.expand_options(pf.to(dev), pb.to(dev), pp.to(dev), pm.to(dev), index.to(dev))
    safe = index.clamp(min=0)
    valid = (index >= 0)
    ef = (pf[safe] * valid[..., None, None]).reshape(bs, K, frames * boxes, F)
    eb = pb[safe] * valid[..., None, None]
    eb[..., 11] = torch.arange(frames).view(1, 1, frames, 1) * valid[..., None]
    ep = (pp[safe] * valid[..., None, None]).reshape(bs, K, frames * boxes, C)
    em = (pm[safe] * valid[..., None]).reshape(bs, K, frames * boxes)
    assert torch.equal(f.cpu(), ef) and torch.equal(bx.cpu(), eb.reshape(bs, K, frames * boxes, 12))
    assert torch.equal(pr.cpu(), ep) and torch.equal(m.cpu(), em)


def test_gemm_splitk_xcd_layout_does_not_change_results(dev, lib):
    """Split-K workgroups are numbered split-major per XCD (decode_tile; option GEMM_SPLIT_MAP = 0 restores the old split-fastest order): the
    layout decides only WHERE a (tile, split) pair runs, so products, fused row sums and a beta = 1 accumulation are bit-identical
    between the two orders."""
    import hashlib
    from ytvln import _lib, ops
    digests = []
    for m in (0, 1):
        prev = _lib.set_option("GEMM_SPLIT_MAP", m)
        try:
            h = hashlib.sha256()
            for (M, N, K, ta, tb) in [(768, 3072, 4480, 1, 0), (1024, 1024, 16128, 1, 0), (768, 768, 4480, 1, 0), (2304, 768, 4480, 1, 0), (1000, 520, 8192, 0, 1)]:
                g = torch.Generator().manual_seed(M + N + K)
                A = torch.randn((K, M) if ta else (M, K), generator=g).to(dev)
                B = torch.randn((N, K) if tb else (K, N), generator=g).to(dev)
                C = torch.randn(M, N, generator=g).to(dev)
                C0 = C.clone()
                rs = torch.empty(M, device=dev)
                done = ops._gemm(A, A.stride(0), ta, B, B.stride(0), tb, C, N, M, N, K, beta=1.0, rowsum=rs if ta else None)
                torch.cuda.synchronize()
                h.update(C.cpu().numpy().tobytes())
                if done:
                    h.update(rs.cpu().numpy().tobytes())
                ref = (A.t() if ta else A).double() @ (B.t() if tb else B).double() + C0.double()
                assert float((C.double() - ref).abs().max()) / float(ref.abs().max()) < 1e-5
            digests.append(h.hexdigest())
        finally:
            _lib.set_option("GEMM_SPLIT_MAP", prev)
    assert digests[0] == digests[1], "the XCD layout of split-K workgroups changed the results"


def test_scatter_add_rows_sorted_is_exact_and_reproducible(dev, lib):
    """Word-embedding gradient without atomics: equals an fp64 index_add to fp32 rounding, skips the padding id, and two launches agree
    bit for bit (the atomic kernel does not guarantee that)."""
    from ytvln._lib import call
    g = torch.Generator().manual_seed(3)
    M, H, V = 4480, 768, 997
    x = torch.randn(M, H, generator=g).to(dev)
    ids = torch.randint(0, V, (M,), generator=g)
    ids[::7] = 103                                      # a long run ([MASK]) and the padding id
    ids[::11] = 0
    ids = ids.to(dev)
    outs = []
    for _ in range(2):
        tg = torch.zeros(V, H, device=dev)
        s, perm = torch.sort(ids, stable=True)
        call("ytvln_scatter_add_rows_sorted_f32", x.data_ptr(), H, s.data_ptr(), perm.data_ptr(), M, H, tg.data_ptr(), 0, None)
        outs.append(tg)
    assert torch.equal(outs[0], outs[1])
    ref = torch.zeros(V, H, dtype=torch.float64, device=dev).index_add_(0, ids, x.double())
    ref[0] = 0
    assert float((outs[0].double() - ref).abs().max()) < 1e-4 and float(outs[0][0].abs().max()) == 0.0


@pytest.mark.parametrize("M,N,K,expect", [(1024, 1024, 16128, True), (768, 3072, 4480, True), (2304, 768, 4480, True), (96, 40, 160, True),
                                           (1601, 1024, 16128, False), (64, 64, 100, False)])
def test_gemm_rowsum_rides_on_the_weight_gradient(dev, lib, M, N, K, expect):
    """ytvln_gemm_f32_rowsum: dW = dY^T X with db = column sums of dY produced by the same launch (split-K and unsplit plans); when the
    launch cannot do it (M-contiguous A with M % 4 != 0 zero-padded / K % 32 != 0 -> generic kernel) it says so and the caller uses colsum.
    Also: the product itself is unchanged by the extra output, and repeated launches are bit-identical (fixed summation order)."""
    import ctypes
    from ytvln import _lib, ops
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    dY = torch.randn(K, M, generator=g).to(dev)          # A operand stored [K, M]: transA = 1
    X = torch.randn(K, N, generator=g).to(dev)
    ref_w = (dY.double().t() @ X.double())
    ref_b = dY.double().sum(0)
    outs = []
    for rep in range(2):
        dW = torch.empty(M, N, device=dev)
        db = torch.full((M,), float("nan"), device=dev)
        done = ops._gemm(dY, M, 1, X, N, 0, dW, N, M, N, K, rowsum=db)
        assert done == expect, (done, expect)
        close(dW, ref_w, 2e-3 * (K / 4096) ** 0.5 + 1e-4, 2e-5, "dW")
        if done:
            close(db, ref_b, 1e-3 * (K / 4096) ** 0.5 + 1e-5, 2e-5, "db from the GEMM")
        else:
            assert bool(torch.isnan(db).all())               # untouched: the caller falls back to colsum
        outs.append((dW.clone(), db.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and (not expect or torch.equal(outs[0][1], outs[1][1]))
    plain = torch.empty(M, N, device=dev)
    ops._gemm(dY, M, 1, X, N, 0, plain, N, M, N, K)
    assert torch.equal(plain, outs[0][0])


# every arm of the tile dispatch of ytvln_gemm_f32, forced through the experiment knobs: (transA, transB, GEMM_TILE, GEMM_SPLITS)
_TILE_DIMS = [(128, 128), (128, 64), (64, 64), (256, 128), (256, 256), (224, 256), (160, 256)]
_SWITCH_CASES = ([(0, tb, t, 1) for tb in (1, 0) for t in range(7)] + [(0, tb, t, 2) for tb in (1, 0) for t in (0, 5, 6)] +
                 [(1, 0, t, 1) for t in (0, 1, 2, 4)] + [(1, 0, t, 2) for t in (0, 4)])
_SWITCH_OPERANDS = {}


def _switch_operands(dev, ta, tb, M, N, K):
    """(A, B, bias or None, fp64 product) of one layout, made once for all its cases."""
    key = (ta, tb)
    if key not in _SWITCH_OPERANDS:
        A = rnd(dev, *((K, M) if ta else (M, K)), seed=11)
        B = rnd(dev, *((N, K) if tb else (K, N)), seed=12)
        bias = None if ta else rnd(dev, N, seed=13)
        ref = (A.t() if ta else A).double() @ (B.t() if tb else B).double()
        _SWITCH_OPERANDS[key] = (A, B, bias, ref if bias is None else ref + bias.double())
    return _SWITCH_OPERANDS[key]


@pytest.mark.parametrize("ta,tb,tile,splits", _SWITCH_CASES)
def test_gemm_tile_dispatch_switch(dev, lib, ta, tb, tile, splits):
    """ytvln_gemm_f32 with GEMM_TILE / GEMM_SPLITS forced, so that every tile of the dispatch runs in every layout that has it, split and
    unsplit, whatever the planner would choose for the shape: M = 500 and N = 264 leave a ragged last tile row and column on every tile,
    K = 1024 is two splits of 512.  The plan is asserted first -- a case must not quietly run 128x128 -- and the entry point is called
    directly: ops._gemm caches the workspace size by shape, and a size cached before the knobs were set would make a forced split run unsplit."""
    import ctypes
    from ytvln import _lib
    M, N, K = 500, 264, 1024
    A, B, bias, ref = _switch_operands(dev, ta, tb, M, N, K)
    prev = (_lib.set_option("GEMM_TILE", tile), _lib.set_option("GEMM_SPLITS", splits))
    try:
        tm, tn, sp = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert _lib.load().ytvln_gemm_plan(M, N, K, ta, 0, ctypes.byref(tm), ctypes.byref(tn), ctypes.byref(sp)) == 0
        assert (tm.value, tn.value, sp.value) == _TILE_DIMS[tile] + (splits,)
        need = int(_lib.load().ytvln_gemm_workspace_elems(M, N, K, 0))
        assert splits == 1 or need >= splits * M * N, need
        ws = torch.empty(need, device=dev) if need else None
        C = torch.full((M, N), float("nan"), device=dev)
        _lib.call("ytvln_gemm_f32", A.data_ptr(), A.stride(0), ta, B.data_ptr(), B.stride(0), tb, C.data_ptr(), N,
                  bias.data_ptr() if bias is not None else None, None, 0, M, N, K, 0, 0.0, ws.data_ptr() if need else None, need, 0, None)
        torch.cuda.synchronize()
    finally:
        _lib.set_option("GEMM_TILE", prev[0])
        _lib.set_option("GEMM_SPLITS", prev[1])
    close(C, ref, 2e-4 * math.sqrt(K / 64) + (0.0 if tb else 1e-5), 1e-4, f"tile {_TILE_DIMS[tile]} x {splits}, transA {ta} transB {tb}")
