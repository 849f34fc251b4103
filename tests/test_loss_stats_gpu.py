"""GPU: label smoothing and same-pass accuracy in the CE / KL loss kernels (ops.cross_entropy_stats, ops.kl_masked_stats, the
`label_smoothing` argument of ops.cross_entropy, args.label_smoothing / args.token_accuracy in the loops) against the fp64 restatement of
tests/loss_stats_ref.py on the same inputs.  Bars: the ones test_kernels_gpu.py::test_losses holds these kernels to -- loss 2e-6 (abs and
rel), gradient relative L2 below 1e-5 -- and row_top / hits / count exactly.  Shapes: V below, at and above one 256-thread sweep, the vision
width 1601, the vocabulary 30522 behind a padded leading dimension; one row, a few rows, more rows than one finalize sweep."""
import functools
import math

import numpy as np
import pytest
import torch

import loss_stats_ref as R
from helpers import args_ns, close, rel_l2

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EPS = (0.0, 0.1, 0.5)
JUNK = 1e30          # in the padding columns of the logits: read by mistake, it would be the arg-max and the whole log-sum-exp


def _bits(t):
    return t.detach().contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


@functools.lru_cache(maxsize=None)
def _ce_inputs(M, V, all_ignored=False):
    g = torch.Generator().manual_seed(1000 * M + V)
    x = torch.randn(M, V, generator=g) * 2.0
    t = torch.randint(0, V, (M,), generator=g)
    t[2::3] = -1                      # every third target ignored
    if M >= 5:
        t[1] = int(x[1].argmax())     # at least one hit and ...
        t[3] = int(x[3].argmin())     # ... one miss, whatever the seed
    if all_ignored:
        t[:] = -1
    return x, t


@functools.lru_cache(maxsize=None)
def _ce_ref(M, V, eps, all_ignored=False):
    x, t = _ce_inputs(M, V, all_ignored)
    return R.ce_stats(x.numpy(), t.numpy(), -1, eps, gout=3.0)


def _padded(x, pad, dev, junk=JUNK, dtype=torch.float32):
    """x on the device as a [M, V] view of a [M, V + pad] buffer whose padding holds junk"""
    M, V = x.shape
    buf = torch.full((M, V + pad), junk, device=dev, dtype=dtype)
    buf[:, :V] = x.to(dev).to(dtype)
    return buf[:, :V]


def _check_ce(dev, M, V, pad, eps, all_ignored=False):
    from ytvln import ops
    x, t = _ce_inputs(M, V, all_ignored)
    ref = _ce_ref(M, V, eps, all_ignored)
    lg = _padded(x, pad, dev).detach().requires_grad_(True)
    loss, hits, count, row_top = ops.cross_entropy_stats(lg, t.to(dev), -1, eps)
    assert loss.requires_grad and not hits.requires_grad and not count.requires_grad and not row_top.requires_grad
    assert hits.shape == count.shape == () and hits.dtype == count.dtype == torch.float32 and row_top.dtype == torch.int64 and row_top.shape == (M,)
    print(f"ce M={M} V={V} eps={eps}: loss {float(loss)!r} ref {ref['loss']!r} hits {float(hits)} count {float(count)}")
    assert np.array_equal(row_top.cpu().numpy(), ref["row_top"])
    assert float(hits) == ref["hits"] and float(count) == ref["count"]
    if all_ignored:
        assert math.isnan(float(loss)) and math.isnan(ref["loss"]) and float(hits) == 0.0 and float(count) == 0.0
        return
    close(loss, ref["loss"], 2e-6, 2e-6, f"ce stats loss M={M} V={V} eps={eps}")
    (loss * 3.0).backward()
    err = rel_l2(lg.grad, ref["grad"])
    print(f"   gradient rel-L2 {err:.3e}")
    assert err < 1e-5, err
    # ops.cross_entropy(label_smoothing=) is the same path
    l2 = ops.cross_entropy(lg.detach(), t.to(dev), -1, label_smoothing=eps)
    if eps != 0.0:
        assert torch.equal(_bits(l2), _bits(loss))
    else:
        close(l2, ref["loss"], 2e-6, 2e-6, "plain ce")


@pytest.mark.parametrize("V", [2, 7, 255, 256, 257, 1601])
@pytest.mark.parametrize("M", [1, 5, 300])
def test_ce_stats_fp32_against_the_fp64_restatement(dev, lib, M, V):
    for eps in EPS:
        _check_ce(dev, M, V, 3, eps)


def test_ce_stats_fp32_vocabulary_behind_a_padded_leading_dimension(dev, lib):
    for eps in EPS:
        _check_ce(dev, 300, 30522, 6, eps)


@pytest.mark.parametrize("M,V", [(1, 7), (5, 257), (300, 1601)])
def test_ce_stats_all_targets_ignored(dev, lib, M, V):
    _check_ce(dev, M, V, 3, 0.1, all_ignored=True)
    _check_ce(dev, M, V, 3, 0.0, all_ignored=True)


@functools.lru_cache(maxsize=None)
def _kl_inputs(M, C, masked="third"):
    g = torch.Generator().manual_seed(2000 * M + C)
    x = torch.randn(M, C, generator=g)
    tt = torch.softmax(torch.randn(M, C, generator=g) * 3, -1)
    mk = torch.ones(M, dtype=torch.int64)
    mk[2::3] = 0
    if M >= 5:
        x[1, int(tt[1].argmax())] = 9.0          # one certain hit ...
        x[3, int(tt[3].argmin())] = 9.0          # ... and one certain miss
        tt[4, : C // 2] = 0.0                    # zero targets add nothing (xlogy)
    if masked == "all":
        mk[:] = 0
    return x, tt, mk


@functools.lru_cache(maxsize=None)
def _kl_ref(M, C, masked="third"):
    x, tt, mk = _kl_inputs(M, C, masked)
    return R.kl_stats(x.numpy(), tt.numpy(), mk.numpy(), gout=3.0)


def _check_kl(dev, M, C, pad, masked="third"):
    from ytvln import ops
    x, tt, mk = _kl_inputs(M, C, masked)
    ref = _kl_ref(M, C, masked)
    pr = _padded(x, pad, dev).detach().requires_grad_(True)
    tg = _padded(tt, pad + 1, dev)
    loss, hits, count, row_top = ops.kl_masked_stats(pr, tg, mk.to(dev))
    assert loss.requires_grad and not hits.requires_grad and not count.requires_grad and not row_top.requires_grad
    print(f"kl M={M} C={C} {masked}: loss {float(loss)!r} ref {ref['loss']!r} hits {float(hits)} count {float(count)}")
    assert np.array_equal(row_top.cpu().numpy(), ref["row_top"])
    assert float(hits) == ref["hits"] and float(count) == ref["count"]
    close(loss, ref["loss"], 2e-6, 2e-6, f"kl stats loss M={M} C={C}")
    (loss * 3.0).backward()
    if masked == "all":
        assert float(loss) == 0.0 and float(hits) == 0.0 and float(count) == 0.0 and float(pr.grad.abs().max()) == 0.0
        return
    err = rel_l2(pr.grad, ref["grad"])
    print(f"   gradient rel-L2 {err:.3e}")
    assert err < 1e-5, err


@pytest.mark.parametrize("C", [2, 7, 255, 256, 257, 1601])
@pytest.mark.parametrize("M", [1, 5, 300])
def test_kl_stats_fp32_against_the_fp64_restatement(dev, lib, M, C):
    _check_kl(dev, M, C, 3)


def test_kl_stats_no_row_masked(dev, lib):
    _check_kl(dev, 5, 257, 3, masked="all")


# ---- 2. ties and special values, planted by hand -----------------------------------------------------------------------------------------
def test_equal_maxima_the_lowest_index_wins(dev, lib):
    """pairs of equal maxima on both sides of a 64-lane boundary (two waves), of a 256-thread boundary (two sweeps of the row), in the same
    thread (two sweeps), and far apart; for the KL the same plants in the target rows"""
    from ytvln import ops
    V = 600
    plants = [(63, 64), (255, 256), (5, 261), (40, 300), (64, 599), (0, 599), (191, 192, 448), (257, 1), (511, 512)]
    g = torch.Generator().manual_seed(7)
    x = torch.randn(len(plants), V, generator=g)
    for r, cols in enumerate(plants):
        x[r, list(cols)] = 50.0
    want = [min(c) for c in plants]
    t = torch.tensor(want)
    t[1] = 256          # the HIGHER of the equal maxima as the target: no hit
    _, hits, count, row_top = ops.cross_entropy_stats(x.to(dev), t.to(dev), -1, 0.1)
    assert row_top.tolist() == want == np.argmax(x.numpy(), -1).tolist()
    assert float(hits) == len(plants) - 1 and float(count) == len(plants)
    # bf16 logits: rounding creates ties the fp32 row does not have; the rule is the same
    xb = x.to(BF)
    _, _, _, top_b = ops.cross_entropy_stats(xb.to(dev), t.to(dev), -1, 0.0)
    assert top_b.tolist() == np.argmax(xb.float().numpy(), -1).tolist()
    # KL: prediction rows against target rows with their own planted ties
    tt = torch.softmax(torch.randn(len(plants), V, generator=g), -1)
    for r, cols in enumerate(plants):
        tt[r, list(cols)] = 0.5
    mk = torch.ones(len(plants), dtype=torch.int64)
    _, hits, count, row_top = ops.kl_masked_stats(x.to(dev), tt.to(dev), mk.to(dev))
    assert row_top.tolist() == want and float(hits) == len(plants) and float(count) == len(plants)
    tt[2, 5], tt[2, 261] = 0.25, 0.5          # the target's maximum moves to the other plant: one hit fewer
    _, hits, _, _ = ops.kl_masked_stats(x.to(dev), tt.to(dev), mk.to(dev))
    assert float(hits) == len(plants) - 1


@pytest.mark.parametrize("V", [7, 600])
def test_a_nan_logit_poisons_its_row_only_and_is_the_arg_max(dev, lib, V):
    """V = 7: the row is narrower than a wave, so the NaN meets threads that hold nothing"""
    from ytvln import ops
    g = torch.Generator().manual_seed(8)
    x = torch.randn(4, V, generator=g)
    t = torch.tensor([1, 2, 3, 4])
    first, second = (3, 5) if V == 7 else (70, 330)
    x[1, first] = x[1, second] = math.nan
    x[1, 0] = 80.0
    for eps in (0.0, 0.1):
        ref = R.ce_stats(x.numpy(), t.numpy(), -1, eps)
        lg = x.to(dev).requires_grad_(True)
        loss, hits, count, row_top = ops.cross_entropy_stats(lg, t.to(dev), -1, eps)
        loss.backward()
        assert math.isnan(float(loss)) and math.isnan(ref["row_loss"][1])
        assert row_top.tolist() == ref["row_top"].tolist() and row_top[1] == first
        assert float(hits) == ref["hits"] and float(count) == 4.0
        grad = lg.grad.cpu()
        assert bool(torch.isnan(grad[1]).all()) and bool(torch.isfinite(grad[[0, 2, 3]]).all())
        assert rel_l2(grad[[0, 2, 3]], ref["grad"][[0, 2, 3]]) < 1e-5          # the NaN stays in its row


def test_ranking_rows_with_minus_inf_tails(dev, lib):
    """[bs, 7] ranking logits as pad_packed leaves them: finite loss, the smoothing mass over the finite classes only, zero gradient in the
    -inf columns; a row whose TARGET column is -inf gives +inf, as ops.cross_entropy does today"""
    from ytvln import ops
    g = torch.Generator().manual_seed(9)
    x = torch.randn(6, 7, generator=g) * 2
    widths = [7, 3, 5, 2, 4, 6]
    t = torch.tensor([0, 2, -1, 1, 3, 5])
    for r, w in enumerate(widths):
        x[r, w:] = -math.inf
    for eps in EPS:
        ref = R.ce_stats(x.numpy(), t.numpy(), -1, eps)
        lg = x.to(dev).requires_grad_(True)
        loss, hits, count, row_top = ops.cross_entropy_stats(lg, t.to(dev), -1, eps)
        loss.backward()
        assert math.isfinite(float(loss))
        close(loss, ref["loss"], 2e-6, 2e-6, f"ranking rows eps={eps}")
        assert row_top.tolist() == ref["row_top"].tolist() and float(hits) == ref["hits"] and float(count) == 5.0
        grad = lg.grad.cpu()
        assert bool((grad[torch.isinf(x)] == 0.0).all())
        assert rel_l2(grad, ref["grad"]) < 1e-5
    t2 = t.clone()
    t2[1] = 5          # row 1 has 3 options: its target's logit is -inf
    for eps in (0.0, 0.1):
        loss = ops.cross_entropy_stats(x.to(dev), t2.to(dev), -1, eps)[0]
        assert float(loss) == math.inf and R.ce_stats(x.numpy(), t2.numpy(), -1, eps)["loss"] == math.inf
    assert float(ops.cross_entropy(x.to(dev), t2.to(dev), -1)) == math.inf
    bad = t.clone()
    bad[0] = 7         # outside [0, V) and not the ignore index: NaN, never an out-of-bounds read
    assert math.isnan(float(ops.cross_entropy_stats(x.to(dev), bad.to(dev), -1, 0.1)[0]))


# ---- 3. eps = 0 is the plain kernel, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("M,V", [(5, 7), (300, 1601), (40, 30522)])
def test_without_smoothing_the_stats_ops_are_the_plain_ops_bit_for_bit(dev, lib, M, V, dtype):
    from ytvln import ops
    x, t = _ce_inputs(M, V)
    t = t.to(dev)
    pad = (-V) % 8 + 8          # a leading dimension the bf16 rows are read through in place
    a = _padded(x, pad, dev, junk=7.0, dtype=dtype).detach().requires_grad_(True)
    b = a.detach().contiguous().requires_grad_(True)          # another leading dimension, the same bits
    la = ops.cross_entropy(a, t, -1)
    lb, _, _, _ = ops.cross_entropy_stats(b, t, -1, 0.0)
    (la * 3.0).backward()
    (lb * 3.0).backward()
    assert torch.equal(_bits(la), _bits(lb)) and a.grad.dtype == b.grad.dtype == dtype and torch.equal(_bits(a.grad), _bits(b.grad))
    if V <= 1601:
        xk, tt, mk = _kl_inputs(M, V)
        p = _padded(xk, pad, dev, junk=7.0, dtype=dtype).detach().requires_grad_(True)
        q = p.detach().contiguous().requires_grad_(True)
        ka = ops.kl_masked(p, tt.to(dev), mk.to(dev))
        kb, _, _, _ = ops.kl_masked_stats(q, tt.to(dev), mk.to(dev))
        (ka * 3.0).backward()
        (kb * 3.0).backward()
        assert torch.equal(_bits(ka), _bits(kb)) and torch.equal(_bits(p.grad), _bits(q.grad))


def test_smoothing_backward_with_eps_zero_writes_what_the_plain_backward_writes(dev, lib):
    from ytvln import _lib
    M, V = 300, 1601
    x, t = _ce_inputs(M, V)
    x, t = x.to(dev), t.to(dev)
    f = lambda *s: torch.empty(*s, device=dev)          # noqa: E731
    row_lse, row_nv, row_loss, out, gout = f(M), f(M), f(M), f(4), torch.full((1,), 3.0, device=dev)
    row_top = torch.empty(M, dtype=torch.int64, device=dev)
    d0, d1 = torch.zeros(M, V, device=dev), torch.zeros(M, V, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    _lib.call("ytvln_ce_stats_fwd_f32", x.data_ptr(), V, t.data_ptr(), -1, 0.0, row_lse.data_ptr(), row_nv.data_ptr(), row_loss.data_ptr(),
              row_top.data_ptr(), out.data_ptr(), M, V, st)
    _lib.call("ytvln_ce_bwd_f32", x.data_ptr(), V, t.data_ptr(), -1, row_lse.data_ptr(), out.data_ptr(), gout.data_ptr(), d0.data_ptr(), V, M, V, st)
    _lib.call("ytvln_ce_smooth_bwd_f32", x.data_ptr(), V, t.data_ptr(), -1, 0.0, row_lse.data_ptr(), row_nv.data_ptr(), out.data_ptr(),
              gout.data_ptr(), d1.data_ptr(), V, M, V, st)
    assert torch.equal(_bits(d0), _bits(d1)) and float(d0.abs().max()) > 0
    live = (t != -1)
    assert bool((row_nv[live] == V).all()) and bool((row_nv[~live] == 0).all())


# ---- 4. bf16 logits: the contract of test_loss_gradients_bf16_and_adamw_copy -----------------------------------------------------------
@pytest.mark.parametrize("eps", EPS)
def test_bf16_logits_loss_of_the_rounded_logits_and_gradient_rounded_once(dev, lib, eps):
    from ytvln import _lib, ops
    M, V, LD = 300, 1601, 1608
    x, t = _ce_inputs(M, V)
    t = t.to(dev)
    buf = torch.full((M, LD), 7.0, device=dev, dtype=BF)          # junk in the padding columns of the logits must not matter
    buf[:, :V] = x.to(dev).to(BF)
    logits_b = buf[:, :V].detach().requires_grad_(True)
    logits = logits_b.detach().float().requires_grad_(True)
    l32, h32, c32, top32 = ops.cross_entropy_stats(logits, t, -1, eps)
    l32.backward()
    lb, hb, cb, topb = ops.cross_entropy_stats(logits_b, t, -1, eps)
    lb.backward()
    gb = logits_b.grad
    assert lb.dtype == torch.float32 and float(lb) == float(l32) and float(hb) == float(h32) and float(cb) == float(c32)
    assert torch.equal(topb, top32)
    assert gb.dtype == BF and gb.shape == (M, V) and torch.equal(gb, logits.grad.to(BF))
    # the gradient buffer as the kernel leaves it: zeros up to the leading dimension
    dl, ldd = ops._alloc_rows_bf16(M, V, dev)
    dl.fill_(3.0)
    full = torch.as_strided(dl, (M, ldd), (ldd, 1))
    full.fill_(3.0)
    f = lambda *s: torch.empty(*s, device=dev)          # noqa: E731
    row_lse, row_nv, row_loss, out, one = f(M), f(M), f(M), f(4), torch.ones(1, device=dev)
    row_top = torch.empty(M, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    _lib.call("ytvln_ce_stats_fwd_bf16", buf.data_ptr(), LD, t.data_ptr(), -1, eps, row_lse.data_ptr(), row_nv.data_ptr(), row_loss.data_ptr(),
              row_top.data_ptr(), out.data_ptr(), M, V, st)
    _lib.call("ytvln_ce_smooth_bwd_bf16", buf.data_ptr(), LD, t.data_ptr(), -1, eps, row_lse.data_ptr(), row_nv.data_ptr(), out.data_ptr(),
              one.data_ptr(), dl.data_ptr(), ldd, M, V, st)
    assert ldd % 8 == 0 and ldd > V and torch.equal(full[:, :V], gb) and float(full[:, V:].float().abs().max()) == 0.0
    assert float(out[0]) == float(lb) and torch.equal(row_top, topb)
    # KL
    xk, tt, mk = _kl_inputs(M, V)
    kbuf = torch.full((M, LD), 7.0, device=dev, dtype=BF)
    kbuf[:, :V] = xk.to(dev).to(BF)
    pred_b = kbuf[:, :V].detach().requires_grad_(True)
    pred = pred_b.detach().float().requires_grad_(True)
    kb, khb, kcb, ktb = ops.kl_masked_stats(pred_b, tt.to(dev), mk.to(dev))
    kb.backward()
    k32, kh, kc, kt = ops.kl_masked_stats(pred, tt.to(dev), mk.to(dev))
    k32.backward()
    assert float(kb) == float(k32) and float(khb) == float(kh) and float(kcb) == float(kc) and torch.equal(ktb, kt)
    assert pred_b.grad.dtype == BF and torch.equal(pred_b.grad, pred.grad.to(BF))


# ---- 5. capture --------------------------------------------------------------------------------------------------------------------------
def test_both_stats_ops_replay_from_one_graph(dev, lib):
    """forward and backward of both ops in one torch.cuda.graph on a single stream, replayed twice with the logits and targets refilled in place"""
    from ytvln import ops
    M, V, C = 37, 1601, 257
    fills = []
    for seed in (1, 2):
        g = torch.Generator().manual_seed(seed)
        t = torch.randint(0, V, (M,), generator=g)
        t[seed::3] = -1
        fills.append((torch.randn(M, V, generator=g).to(dev), t.to(dev), torch.randn(M, C, generator=g).to(dev),
                      torch.softmax(torch.randn(M, C, generator=g) * 3, -1).to(dev), (torch.rand(M, generator=g) < 0.6).long().to(dev)))

    def run(x, t, p, tt, mk):
        x.grad = p.grad = None
        l1, h1, c1, r1 = ops.cross_entropy_stats(x, t, -1, 0.1)
        l2, h2, c2, r2 = ops.kl_masked_stats(p, tt, mk)
        (l1 + 2.0 * l2).backward()
        return [l1.detach(), h1, c1, r1, l2.detach(), h2, c2, r2, x.grad, p.grad]

    eager = []
    for f in fills:
        x, t, p, tt, mk = (a.clone() for a in f)
        eager.append([o.clone() for o in run(x.requires_grad_(True), t, p.requires_grad_(True), tt, mk)])
    x, t, p, tt, mk = (a.clone() for a in fills[0])
    x.requires_grad_(True), p.requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(x, t, p, tt, mk)          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(x, t, p, tt, mk)
    for f, want in ((fills[1], eager[1]), (fills[0], eager[0])):
        with torch.no_grad():
            for dst, src in zip((x, t, p, tt, mk), f):
                dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        for got, w in zip(outs, want):
            assert got.dtype == w.dtype and torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got,
                                                        w.view(torch.int32) if w.dtype == torch.float32 else w)


# ---- 6. the loops on the micro config --------------------------------------------------------------------------------------------------
NEW = ("ytvln_ce_stats_fwd", "ytvln_ce_smooth_bwd", "ytvln_kl_stats_fwd")


def _micro(dev, **settings):
    """the micro model with the three objectives whose loss is finite on a batch with option holes (the ranking logits then carry -inf)"""
    from test_model_gpu import build_lily
    args = args_ns(ranking=True, traj_judge=False, masked_vision=True, masked_language=True)
    for k, v in settings.items():
        setattr(args, k, v)
    model, _ = build_lily(dev, "micro.json", args, seed=11)
    return model.train(), args


def _micro_batch(dev):
    from ytvln import synth
    return synth.to_torch(synth.make_batch(bs=2, K=3, T=8, frames=2, boxes=3, F=16, C=11, vocab=97, seed=21, opt_holes=1, ignore_rank_frac=0.0), dev)


def _step(dev, monkeypatch=None, aware=False, **settings):
    """one forward + backward of train_step -> (loss, metrics, {name: grad}, names of the entry points launched)"""
    from ytvln import ops
    from ytvln import utils_init as U
    model, args = _micro(dev, **settings)
    batch = _micro_batch(dev)
    names = []
    if monkeypatch is not None:
        real = ops.call
        monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    loss, metrics = U.train_step(model, None, None, batch, args, 0, all_options=bool(batch[13].all()), loss_aware_heads=aware, capacity_frac=0.5,
                                 optimizer_step=False)
    torch.cuda.synchronize()
    if monkeypatch is not None:
        monkeypatch.undo()
    return loss, metrics, {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}, names


@functools.lru_cache(maxsize=None)
def _micro_reference(eps):
    """the restatement on the micro model's own logits (a separate forward of the same model and batch)"""
    from ytvln import utils_init as U
    dev = torch.device("cuda", 0)
    model, args = _micro(dev)
    batch = _micro_batch(dev)
    with torch.no_grad():
        out = model(*U.get_model_input(batch, bool(batch[13].all())))
    lang = out["language"].reshape(-1, out["language"].shape[-1]).cpu().numpy()
    vis = out["vision"].reshape(-1, out["vision"].shape[-1]).cpu().numpy()
    vt, vm = U.get_vision_target(batch, bool(batch[13].all()))
    rank = U.pad_packed(out["ranking"].squeeze(1), batch[13]).cpu().numpy()
    return dict(language=R.ce_stats(lang, U.get_linguistic_target(batch, bool(batch[13].all())).cpu().numpy(), -1, eps),
                vision=R.kl_stats(vis, vt.float().cpu().numpy(), vm.cpu().numpy()),
                ranking=R.ce_stats(rank, batch[0].cpu().numpy(), -1, eps))


def _acc(ref):
    return float(np.float32(ref["hits"]) / np.float32(max(ref["count"], 1)))


def test_train_step_with_both_settings_off_launches_nothing_new(dev, lib, monkeypatch):
    loss, metrics, grads, names = _step(dev, monkeypatch)
    assert names and not [n for n in names if n.startswith(NEW)]
    assert {"ytvln_ce_fwd_f32", "ytvln_ce_bwd_f32", "ytvln_kl_fwd_f32", "ytvln_kl_bwd_f32"} <= set(names)
    assert set(metrics) == {"loss", "accuracy"} and set(metrics["accuracy"]) == {"ranking"}
    assert set(metrics["loss"]) == {"vision", "language", "ranking"} and math.isfinite(float(loss))
    # explicit defaults are the same step
    loss2, metrics2, grads2, names2 = _step(dev, monkeypatch, label_smoothing=0.0, token_accuracy=False)
    assert names2 == names and torch.equal(_bits(loss), _bits(loss2))


def test_token_accuracy_adds_two_exact_accuracies_and_changes_no_bit(dev, lib, monkeypatch):
    off_loss, off_metrics, off_grads, _ = _step(dev)
    loss, metrics, grads, names = _step(dev, monkeypatch, token_accuracy=True)
    assert {"ytvln_ce_stats_fwd_f32", "ytvln_kl_stats_fwd_f32"} <= set(names) and "ytvln_ce_smooth_bwd_f32" not in names
    assert "ytvln_kl_fwd_f32" not in names          # the stats forward replaces the plain one, it is not a second pass
    ref = _micro_reference(0.0)
    assert set(metrics["accuracy"]) == {"ranking", "language", "vision"}
    print({k: float(v) for k, v in metrics["accuracy"].items()}, {k: (v["hits"], v["count"]) for k, v in ref.items()})
    assert ref["language"]["count"] > 0 and ref["vision"]["count"] > 0
    assert float(metrics["accuracy"]["language"]) == _acc(ref["language"])
    assert float(metrics["accuracy"]["vision"]) == _acc(ref["vision"])
    assert float(metrics["accuracy"]["ranking"]) == float(off_metrics["accuracy"]["ranking"]) == ref["ranking"]["hits"] / 2.0
    assert torch.equal(_bits(loss), _bits(off_loss)) and math.isfinite(float(loss))
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    for k in off_metrics["loss"]:
        assert torch.equal(_bits(metrics["loss"][k]), _bits(off_metrics["loss"][k])), k
    assert set(grads) == set(off_grads)
    for n in grads:
        assert torch.equal(_bits(grads[n]), _bits(off_grads[n])), n


def test_label_smoothing_reaches_the_language_and_the_training_ranking_loss_only(dev, lib, monkeypatch):
    off_loss, off_metrics, _, _ = _step(dev)
    loss, metrics, grads, names = _step(dev, monkeypatch, label_smoothing=0.1)
    assert {"ytvln_ce_stats_fwd_f32", "ytvln_ce_smooth_bwd_f32"} <= set(names) and "ytvln_kl_stats_fwd_f32" not in names
    assert set(metrics["accuracy"]) == {"ranking"}
    ref = _micro_reference(0.1)
    assert torch.equal(_bits(metrics["loss"]["vision"]), _bits(off_metrics["loss"]["vision"]))          # untouched, bit for bit
    assert abs(float(off_metrics["loss"]["vision"]) - ref["vision"]["loss"]) <= 1e-4
    want = ref["vision"]["loss"] + ref["language"]["loss"] + ref["ranking"]["loss"]
    print(f"total {float(loss)!r} restatement {want!r}; language {float(metrics['loss']['language'])!r} / {ref['language']['loss']!r}; "
          f"ranking {float(metrics['loss']['ranking'])!r} / {ref['ranking']['loss']!r}")
    assert math.isfinite(want) and abs(float(loss) - want) <= 1e-4
    assert abs(float(metrics["loss"]["language"]) - ref["language"]["loss"]) <= 1e-4
    assert abs(float(metrics["loss"]["ranking"]) - ref["ranking"]["loss"]) <= 1e-4
    assert abs(float(loss) - float(off_loss)) > 1e-3          # and it is not the unsmoothed loss
    assert float(metrics["accuracy"]["ranking"]) == float(off_metrics["accuracy"]["ranking"])
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())


def test_loss_aware_heads_honour_both_settings(dev, lib):
    full_loss, full, _, _ = _step(dev, label_smoothing=0.1, token_accuracy=True)
    aware_loss, aware, _, _ = _step(dev, aware=True, label_smoothing=0.1, token_accuracy=True)
    assert float(aware["head_row_overflow"]) == 0.0
    assert set(aware["accuracy"]) == set(full["accuracy"]) == {"ranking", "language", "vision"}
    for k in full["accuracy"]:
        assert float(aware["accuracy"][k]) == float(full["accuracy"][k]), k
    for k in full["loss"]:          # the bar of test_loss_aware_heads_match_full_heads
        a, b = float(full["loss"][k]), float(aware["loss"][k])
        assert abs(a - b) < 2e-6 * max(1.0, abs(a)), (k, a, b)
    assert abs(float(full_loss) - float(aware_loss)) < 2e-6 * max(1.0, abs(float(full_loss)))
    # label_smoothing = 0: token_accuracy changes no bit on the selected rows either
    l0, m0, g0, _ = _step(dev, aware=True)
    l1, m1, g1, _ = _step(dev, aware=True, token_accuracy=True)
    assert torch.equal(_bits(l0), _bits(l1)) and all(torch.equal(_bits(g0[n]), _bits(g1[n])) for n in g0)
