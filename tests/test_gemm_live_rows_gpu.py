"""GPU: the weight-gradient GEMM that contracts over a device-side list of live rows (ytvln_live_rows_list + ytvln_gemm_f32_live), alone.

dW[M, N] = A^T B with A stored [K, M] (transA = 1), B stored [K, N]; the list names the rows of the contraction that can be non-zero in A.
Operands: listed-out rows of A are zero, listed-out rows of B hold 1e30, so any read that should not contribute shows.  Reference: the
fp64 product over the listed rows.  Bar: max error of the listed launch <= 2 x the max error of the UNLISTED launch on the same operands
(both measured here): the listed sum has fewer terms and should not be worse.

Sparse lists: with fewer than 32 live rows per split the kernel gives every split its share of the rows as one padded tile.  Packed into
whole tiles, 31-33 live rows were ONE serial chain of 32 products where the unlisted launch adds 4-8 short chains and then the partials,
and four such cases measured 2.18-2.49 x the unlisted error; spread over the splits they measure 0.7-1.0 x (MI355X; the largest ratio of
all 54 cases is 1.5, the splits + 1 tiles of "empty-splits")."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (M, N, K, forced options, expected tile, minimum splits): the smallest shapes that reach each path of the listed kernel
SHAPES = [
    pytest.param(512, 256, 2048, {"GEMM_TILE": 4}, 256, 2, id="256x256-split"),          # (the planner's own pick only from the headline sizes up)
    pytest.param(128, 256, 2048, {}, 128, 2, id="128x128-split"),
    pytest.param(256, 256, 256, {"GEMM_TILE": 4, "GEMM_SPLITS": 1}, 256, 1, id="256x256-unsplit"),
    pytest.param(128, 128, 256, {"GEMM_TILE": 0, "GEMM_SPLITS": 1}, 128, 1, id="128x128-unsplit"),
    pytest.param(320, 200, 1024, {"GEMM_TILE": 4}, 256, 2, id="256x256-ragged-MN"),
    pytest.param(200, 72, 1024, {"GEMM_TILE": 0}, 128, 2, id="128x128-ragged-MN"),
]


def _plan(lib, M, N, K):
    tm, tn, sp = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.ytvln_gemm_plan(M, N, K, 1, 0, ctypes.byref(tm), ctypes.byref(tn), ctypes.byref(sp)) == 0
    return tm.value, tn.value, sp.value


def _masks(K, splits, rng):
    """name -> bool[K]: the lists of the issue."""
    out = {"none": np.zeros(K, bool), "all": np.ones(K, bool)}
    for c in (1, 31, 32, 33):
        m = np.zeros(K, bool)
        m[rng.choice(K, c, replace=False)] = True
        out[f"count{c}"] = m
    m = np.zeros(K, bool)          # splits + 1 k-tiles: two per split, so the later half of the splits has none (count1 leaves all but one empty)
    m[rng.choice(K, 32 * (splits + 1), replace=False)] = True
    out["empty-splits"] = m
    out["half"] = rng.random(K) < 0.5
    m = np.zeros(K, bool)          # frame-shaped runs, as synth.make_batch pads: per item a valid prefix of whole frames
    L = K // 8
    for b in range(8):
        m[b * L: b * L + (L // 8) * int(rng.integers(4, 9))] = True
    out["frames"] = m
    return out


def _expected_list(mask):
    K = mask.size
    live = np.flatnonzero(mask)
    dead = np.flatnonzero(~mask)
    pad = dead[0] if dead.size else K - 1
    return np.concatenate([live, np.full(K + 32 - live.size, pad)]).astype(np.int32), live.size


LISTS = ("none", "all", "count1", "count31", "count32", "count33", "empty-splits", "half", "frames")
_CACHE = {}


def _operands(dev, M, N, K, splits):
    """Per shape, made once and left unchanged: the random operands and the masks of every list."""
    key = (M, N, K)
    if key not in _CACHE:
        rng = np.random.default_rng(M * 7 + N * 3 + K)
        g = torch.Generator(device="cpu").manual_seed(M + N + K)
        _CACHE[key] = (torch.randn(K, M, generator=g).to(dev), torch.randn(K, N, generator=g).to(dev), _masks(K, splits, rng))
    return _CACHE[key]


@pytest.mark.parametrize("name", LISTS)
@pytest.mark.parametrize("M,N,K,force,tile,min_splits", SHAPES)
def test_listed_launch_against_fp64_and_the_unlisted_launch(dev, lib, M, N, K, force, tile, min_splits, name):
    from ytvln import _lib, ops
    prev = {k: _lib.set_option(k, v) for k, v in force.items()}
    try:
        tm, tn, sp = _plan(lib, M, N, K)
        assert (tm, tn) == (tile, tile) and (sp >= 2 if min_splits >= 2 else sp == 1), (tm, tn, sp)
        A0, B0, masks = _operands(dev, M, N, K, sp)
        mask = masks[name]
        mt = torch.from_numpy(mask).to(dev)
        lr = ops.live_rows(mt)
        want_idx, want_count = _expected_list(mask)
        assert int(lr.count.item()) == want_count
        assert np.array_equal(lr.idx.cpu().numpy(), want_idx)
        A = torch.where(mt[:, None], A0, torch.zeros((), device=dev))
        B = torch.where(mt[:, None], B0, torch.full((), 1e30, device=dev))
        ref_w = A[mt].double().t() @ B[mt].double()
        ref_b = A[mt].double().sum(0)

        def launch(live):
            dW = torch.full((M, N), float("nan"), device=dev)
            db = torch.full((M,), float("nan"), device=dev)
            assert ops._gemm(A, M, 1, B, N, 0, dW, N, M, N, K, rowsum=db, live=live) is True
            return dW, db

        pw, pb = launch(None)
        lw, lb = launch(lr)
        lw2, lb2 = launch(lr)
        assert torch.equal(lw, lw2) and torch.equal(lb, lb2), "two listed launches differ"
        e_plain, e_list = float((pw.double() - ref_w).abs().max()), float((lw.double() - ref_w).abs().max())
        s_plain, s_list = float((pb.double() - ref_b).abs().max()), float((lb.double() - ref_b).abs().max())
        print(f"{M}x{N}x{K} tile {tile} splits {sp} list {name} count {want_count}: dW err listed {e_list:.3e} unlisted {e_plain:.3e}; "
              f"row sums listed {s_list:.3e} unlisted {s_plain:.3e}")
        assert bool(torch.isfinite(lw).all()) and bool(torch.isfinite(lb).all())
        if name == "none":
            assert float(lw.abs().max()) == 0.0 and float(lb.abs().max()) == 0.0
        if name == "all":
            assert torch.equal(lw, pw) and torch.equal(lb, pb), "identity list: not the bits of the unlisted launch"
        assert e_list <= 2.0 * e_plain, (e_list, e_plain)
        assert s_list <= 2.0 * s_plain, (s_list, s_plain)
    finally:
        for k, v in prev.items():
            _lib.set_option(k, v)


def test_option_off_and_rows_not_a_multiple_of_32_ignore_the_list(dev, lib):
    """GEMM_LIVE_ROWS = 0, and K % 32 != 0 (the launch leaves the LDS-DMA loop): the list is ignored and the result is the unlisted launch's,
    bit for bit -- also with a list that names NO row, which a launch that read it would answer with zeros."""
    from ytvln import _lib, ops
    g = torch.Generator(device="cpu").manual_seed(5)
    for K, opt in ((2048, 0), (2000, 1)):
        M, N = 256, 128
        A = torch.randn(K, M, generator=g).to(dev)
        B = torch.randn(K, N, generator=g).to(dev)
        lr = ops.live_rows(torch.zeros(K, dtype=torch.bool, device=dev))
        assert int(lr.count.item()) == 0
        prev = _lib.set_option("GEMM_LIVE_ROWS", opt)
        try:
            outs = []
            for live in (None, lr):
                dW = torch.empty(M, N, device=dev)
                db = torch.zeros(M, device=dev)
                ops._gemm(A, M, 1, B, N, 0, dW, N, M, N, K, rowsum=db, live=live)
                outs.append((dW, db))
        finally:
            _lib.set_option("GEMM_LIVE_ROWS", prev)
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), K
        assert float(outs[1][0].abs().max()) > 0.0
