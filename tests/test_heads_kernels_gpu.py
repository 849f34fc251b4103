"""The kernels of csrc/heads.hip on the GPU against fp64 torch on the same inputs: weight normalisation with dim = None (forward, backward,
bf16 copy, the reference's known answers) and the one-feature Linear over rows (fp32 and bf16 rows, dropout, region mask, gradients), their
run-to-run bit identity and their capture into a hipGraph.

Bars: rel-L2 < 1e-5 for every fp32 result -- what tests/test_kernels_gpu.py holds the sibling fp32 streaming kernels to --; the bf16 dx within
2^-8 (one bf16 rounding is at most 2^-9 relative per element; twice that); a masked row within 2e-3 of fl32((dot + b) - 10000), two fp32 ulps
at 1e4.  Each figure is printed before it is asserted."""
import pytest
import torch

from helpers import gold, rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F32_BAR, BF16_DX_BAR, MASKED_BAR = 1e-5, 2.0 ** -8, 2e-3


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _randn(dev, *shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dev)


def _p(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------------------------
# weight normalisation
# ------------------------------------------------------------------------------------------------------------------
def wn_fwd(v, g, want_bf16=True):
    from ytvln import _lib
    n = v.numel()
    w = torch.full_like(v, float("nan"))
    wb = torch.zeros(n, dtype=BF, device=v.device) if want_bf16 else None
    stat = torch.full((2,), float("nan"), device=v.device)
    ws = torch.empty(_lib.load().ytvln_weight_norm_workspace_elems(n), device=v.device)
    _lib.call("ytvln_weight_norm_fwd_f32", _p(v), _p(g), n, _p(w), _p(wb), _p(stat), _p(ws), _stream())
    return w, wb, stat


def wn_bwd(v, dw, stat):
    from ytvln import _lib
    n = v.numel()
    dv, dg = torch.full_like(v, float("nan")), torch.full((), float("nan"), device=v.device)
    ws = torch.empty(_lib.load().ytvln_weight_norm_workspace_elems(n), device=v.device)
    _lib.call("ytvln_weight_norm_bwd_f32", _p(v), _p(dw), _p(stat), n, _p(dv), _p(dg), _p(ws), _stream())
    return dv, dg


def wn_ref64(v, g, dw):
    vd, gd = v.double().cpu().requires_grad_(True), g.double().cpu().requires_grad_(True)
    norm = vd.norm()
    w = vd * (gd / norm)
    (w * dw.double().cpu()).sum().backward()
    return w.detach(), vd.grad, gd.grad, torch.stack([norm.detach(), (gd / norm).detach()])


@pytest.mark.parametrize("n", [4, 7 * 64, 64 * 32 + 4, 1024 * 2048])
def test_weight_norm_against_fp64(dev, lib, n):
    """n = 4: less than one vector per wave; 7 * 64: a ragged tail of vectors; 64 * 32 + 4: three workgroups, the last nearly empty; 1024 * 2048:
    the real size (256 workgroups).  dw = noise + v / std(v), so that <dw, v> -- and with it dg -- is a well-conditioned sum."""
    v = _randn(dev, n, seed=n, scale=0.05)
    g = torch.tensor(1.5, device=dev)
    dw = _randn(dev, n, seed=n + 1) + v / 0.05
    w, wb, stat = wn_fwd(v, g)
    dv, dg = wn_bwd(v, dw, stat)
    w_ref, dv_ref, dg_ref, stat_ref = wn_ref64(v, g, dw)
    errs = dict(w=rel_l2(w, w_ref), dv=rel_l2(dv, dv_ref), dg=rel_l2(dg, dg_ref), stat=rel_l2(stat, stat_ref))
    print(f"[weight_norm n={n}] rel-L2 {errs}")
    assert all(e < F32_BAR for e in errs.values()), errs
    assert torch.equal(wb.view(torch.int16), w.bfloat16().view(torch.int16)), "w_bf16 is not the round-to-nearest-even copy of w"
    w2, wb2, stat2 = wn_fwd(v, g)
    dv2, dg2 = wn_bwd(v, dw, stat2)
    assert torch.equal(w, w2) and torch.equal(wb.view(torch.int16), wb2.view(torch.int16)) and torch.equal(stat, stat2)
    assert torch.equal(dv, dv2) and torch.equal(dg, dg2)
    w3, _, _ = wn_fwd(v, g, want_bf16=False)          # the bf16 copy is optional and changes nothing else
    assert torch.equal(w, w3)


def test_weight_norm_known_answers(dev, lib):
    """w, dv and dg of the reference's weight-normed Linear (g21_weight_norm_kats: [7, 64] and [64, 32], g = 1.5 and -0.75)."""
    k = gold("g21_weight_norm_kats.npz")
    cases = sorted({f.rsplit("/", 1)[0] for f in k.files})
    assert len(cases) == 4
    for c in cases:
        v, dw = torch.from_numpy(k[c + "/v"]).to(dev), torch.from_numpy(k[c + "/dw"]).to(dev)
        g = torch.tensor(float(k[c + "/g"]), device=dev)
        w, _, stat = wn_fwd(v.reshape(-1), g)
        dv, dg = wn_bwd(v.reshape(-1), dw.reshape(-1), stat)
        errs = dict(w=rel_l2(w.view_as(v), k[c + "/w"]), dv=rel_l2(dv.view_as(v), k[c + "/dv"]), dg=rel_l2(dg, k[c + "/dg"]))
        print(f"[weight_norm KAT {c}] rel-L2 {errs}")
        assert all(e < F32_BAR for e in errs.values()), (c, errs)


# ------------------------------------------------------------------------------------------------------------------
# row logit
# ------------------------------------------------------------------------------------------------------------------
def _rows(dev, rows, H, ld, dtype, seed):
    """[rows, H] values in a buffer of leading dimension ld (pad columns NaN: a kernel that reads them shows)."""
    buf = torch.full((rows, ld), float("nan"), dtype=dtype, device=dev)
    buf[:, :H] = _randn(dev, rows, H, seed=seed).to(dtype)
    return buf[:, :H]


def rl_fwd(x, w, bias, mask, p=0.0, rng=None, site=0):
    from ytvln import _lib
    rows, H = x.shape
    out = torch.full((rows,), float("nan"), device=x.device)
    _lib.call("ytvln_row_logit_fwd_" + ("bf16" if x.dtype == BF else "f32"), x.data_ptr(), x.stride(0), _p(w), _p(bias), _p(mask), _p(out), rows, H,
              float(p), _p(rng), site, _stream())
    return out


def rl_bwd(x, w, dy, p=0.0, rng=None, site=0, want_db=True, lddx=None):
    from ytvln import _lib
    rows, H = x.shape
    lddx = lddx or H
    dxb = torch.full((rows, lddx), float("nan"), dtype=x.dtype, device=x.device)
    dw = torch.full((H,), float("nan"), device=x.device)
    db = torch.full((1,), float("nan"), device=x.device) if want_db else None
    ws = torch.empty(_lib.load().ytvln_row_logit_workspace_elems(rows, H), device=x.device)
    _lib.call("ytvln_row_logit_bwd_" + ("bf16" if x.dtype == BF else "f32"), x.data_ptr(), x.stride(0), _p(w), _p(dy), rows, H, float(p), _p(rng), site,
              dxb.data_ptr(), lddx, _p(dw), _p(db), _p(ws), _stream())
    return dxb[:, :H], dw, db


def rl_ref64(x, w, bias, dy, keep=None):
    """fp64 on the values the kernel reads (bf16 rows widened exactly); keep = the [rows, H] keep-scales or None."""
    xd = x.double().cpu() * (keep.double().cpu() if keep is not None else 1.0)
    wd, dyd = w.double().cpu(), dy.double().cpu()
    out = xd @ wd + (bias.double().cpu() if bias is not None else 0.0)
    dx = dyd[:, None] * wd[None, :] * (keep.double().cpu() if keep is not None else 1.0)
    return out, dx, (dyd[:, None] * xd).sum(0), dyd.sum()


def _region_mask(dev, rows):
    m = torch.ones(rows, device=dev)
    m[rows // 2::3] = 0.0          # (rows = 1: the single row is masked)
    return m


def _check_masked(out_m, out_plain, ref_out, mask):
    """Masked rows = fl32((dot + b) - 10000) within 2e-3; unmasked rows are the run without a mask, bit for bit."""
    masked = mask.cpu() == 0
    want = (ref_out[masked] - 10000.0).float().double()
    worst = float((out_m.double().cpu()[masked] - want).abs().max()) if bool(masked.any()) else 0.0
    assert worst <= MASKED_BAR, worst
    assert torch.equal(out_m.cpu()[~masked], out_plain.cpu()[~masked])
    return worst


@pytest.mark.parametrize("dtype,H", [(torch.float32, h) for h in (48, 256, 768, 1024, 2048)] + [(BF, h) for h in (64, 256, 768, 1024, 2048)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_row_logit_against_fp64(dev, lib, dtype, H):
    """rows = 1: one row (three idle waves); 5: a second forward workgroup with one row, a backward run whose waves hold 2 / 1 / 1 / 1 rows; 37: a
    ragged last workgroup and three dw runs; 1000: 63 dw runs.  Every size with bias and with / without mask; 37 rows also without bias;
    5 rows also with ldx = lddx = H + 8."""
    dx_bar = BF16_DX_BAR if dtype == BF else F32_BAR
    w = _randn(dev, H, seed=H, scale=H ** -0.5)
    bias = torch.tensor([0.37], device=dev)
    for rows in (1, 5, 37, 1000):
        dy = _randn(dev, rows, seed=rows + 3) + 0.5          # a mean: db = sum(dy) is a well-conditioned sum
        for ld in ([H, H + 8] if rows == 5 else [H]):
            x = _rows(dev, rows, H, ld, dtype, seed=rows * 7 + H)
            mask = _region_mask(dev, rows)
            ref_out, ref_dx, ref_dw, ref_db = rl_ref64(x, w, bias, dy)
            out = rl_fwd(x, w, bias, None)
            out_m = rl_fwd(x, w, bias, mask)
            dx, dw, db = rl_bwd(x, w, dy, lddx=ld)
            errs = dict(out=rel_l2(out, ref_out), dx=rel_l2(dx, ref_dx), dw=rel_l2(dw, ref_dw), db=rel_l2(db[0], ref_db))
            worst = _check_masked(out_m, out, ref_out, mask)
            print(f"[row_logit {dtype} H={H} rows={rows} ld={ld}] rel-L2 {errs}, masked rows max abs {worst:.2e}")
            assert out.dtype == torch.float32 and dx.dtype == dtype
            assert errs["out"] < F32_BAR and errs["dw"] < F32_BAR and errs["db"] < F32_BAR and errs["dx"] < dx_bar, errs
            if rows == 37:          # without bias (and without db), without mask
                ref_nb = rl_ref64(x, w, None, dy)[0]
                out_nb = rl_fwd(x, w, None, None)
                dx2, dw2, db2 = rl_bwd(x, w, dy, want_db=False)
                assert rel_l2(out_nb, ref_nb) < F32_BAR and db2 is None
                assert torch.equal(dx2, dx) and torch.equal(dw2, dw)
                _check_masked(rl_fwd(x, w, None, mask), out_nb, ref_nb, mask)
            if rows == 1000:          # two launches: the same bits, dw included
                assert torch.equal(rl_fwd(x, w, bias, mask), out_m)
                dx3, dw3, db3 = rl_bwd(x, w, dy)
                assert torch.equal(dx3, dx) and torch.equal(dw3, dw) and torch.equal(db3, db)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_row_logit_dropout_is_the_dropout_kernels_mask(dev, lib, dtype):
    """p = 0.3, H = 256, rows = 37 (ldx = H + 8 as well): the keep-scales are those ytvln_dropout_f32 applies to an fp32 tensor of ones of
    rows * H elements with the same (rng, site) -- whatever the row type and ldx --, in the forward and in the backward alike."""
    from ytvln import _lib
    rows, H, p, site = 37, 256, 0.3, 5
    rng = torch.tensor([20240229, 3], dtype=torch.int64, device=dev)
    ones = torch.ones(rows * H, device=dev)
    keep = torch.empty_like(ones)
    _lib.call("ytvln_dropout_f32", _p(ones), _p(keep), rows * H, p, _p(rng), site, _stream())
    keep = keep.view(rows, H)
    dropped = keep == 0
    frac = float(dropped.float().mean())
    assert 0.25 < frac < 0.35 and bool(((keep == 0) | ((keep - 1.0 / 0.7).abs() < 1e-6)).all()), frac
    w = _randn(dev, H, seed=1, scale=H ** -0.5)
    bias = torch.tensor([-0.2], device=dev)
    dy = _randn(dev, rows, seed=2) + 0.5
    mask = _region_mask(dev, rows)
    for ld in (H, H + 8):
        x = _rows(dev, rows, H, ld, dtype, seed=3)
        ref_out, ref_dx, ref_dw, ref_db = rl_ref64(x, w, bias, dy, keep)
        out = rl_fwd(x, w, bias, None, p, rng, site)
        out_m = rl_fwd(x, w, bias, mask, p, rng, site)
        dx, dw, db = rl_bwd(x, w, dy, p, rng, site, lddx=ld)
        errs = dict(out=rel_l2(out, ref_out), dx=rel_l2(dx, ref_dx), dw=rel_l2(dw, ref_dw), db=rel_l2(db[0], ref_db))
        print(f"[row_logit dropout {dtype} ld={ld}] dropped {frac:.3f}, rel-L2 {errs}")
        assert errs["out"] < F32_BAR and errs["dw"] < F32_BAR and errs["db"] < F32_BAR
        assert errs["dx"] < (BF16_DX_BAR if dtype == BF else F32_BAR)
        assert bool((dx[dropped] == 0).all()) and bool((dx[~dropped] != 0).all())
        _check_masked(out_m, out, ref_out, mask)
        assert not torch.equal(rl_fwd(x, w, bias, None, p, rng, site + 1), out)          # another site: another mask
        assert torch.equal(rl_fwd(x, w, bias, None, p, rng, site), out)


class _FixedDrop:
    """A DropoutState stand-in whose (seed, counter) tensor and site do not move: the same mask in the captured and in the eager run."""

    def __init__(self, tensor, site):
        self.tensor, self._site = tensor, site

    def next_site(self):
        return self._site


def test_heads_ops_capture_into_one_graph(dev, lib):
    """ops.weight_norm -> ops.linear -> ops.row_logit (dropout 0.3, region mask), forward and backward, captured in one torch.cuda.graph on one
    stream; replayed on new input contents it gives what an eager run on those contents gives, bit for bit."""
    from ytvln import ops
    rows, K, N = 37, 64, 64
    rng = torch.tensor([99, 1], dtype=torch.int64, device=dev)
    leaves = [t.requires_grad_(True) for t in (_randn(dev, rows, K, seed=1), _randn(dev, N, K, seed=2, scale=0.1), torch.tensor(1.25, device=dev),
                                               _randn(dev, N, seed=3, scale=0.1), _randn(dev, 1, N, seed=4, scale=0.1), _randn(dev, 1, seed=5))]
    x, v, g, b, wl, bl = leaves
    mask = _region_mask(dev, rows)
    dy = _randn(dev, rows, 1, seed=6)

    def run():
        h = ops.linear(x, ops.weight_norm(v, g), b)
        out = ops.row_logit(h, wl, bl, mask, 0.3, True, _FixedDrop(rng, 7))
        return (out,) + torch.autograd.grad(out, leaves, dy)

    run()          # (code objects loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    with torch.no_grad():
        x.copy_(_randn(dev, rows, K, seed=11))
        dy.copy_(_randn(dev, rows, 1, seed=12))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in captured]
    eager = run()
    torch.cuda.synchronize()
    assert len(replayed) == 7 and replayed[3].shape == ()
    for i, (a, e) in enumerate(zip(replayed, eager)):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, e), i
    # and it is the new contents that were used: against fp64
    keep = torch.empty(rows * N, device=dev)
    ops.call("ytvln_dropout_f32", _p(torch.ones(rows * N, device=dev)), _p(keep), rows * N, 0.3, _p(rng), 7, _stream())
    hd = x.detach().double() @ (v.detach().double() * (g.detach().double() / v.detach().double().norm())).t() + b.detach().double()
    ref = (hd * keep.view(rows, N).double()) @ wl.detach().double().view(-1) + bl.detach().double() + (1.0 - mask.double()) * -10000.0
    open_rows = (mask == 1).cpu()
    assert rel_l2(replayed[0].view(-1).cpu()[open_rows], ref.cpu()[open_rows]) < 1e-4
