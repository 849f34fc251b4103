"""GPU: the forward / input-gradient GEMM whose M dimension runs over a device-side row list (ytvln_live_rows_perm + ytvln_gemm_f32_rows), alone.

C[M, N] = A[M, K] op(B) (transA = 0, both B layouts); position p of the list is row perm[p] of A, C and aux, the first `count` positions are
computed, the rows behind them are dead: exact zeros with beta = 0, untouched with beta != 0.  A (and aux where it is an input) holds NaN on
the dead rows, C (and aux where it is an output) is pre-filled with NaN (beta = 0) or a sentinel pattern (beta = 1), so any read or write that
should not happen shows.  Reference: the UNLISTED launch forced to the same plan on the same operands with finite dead rows -- a listed row
must carry its bits.  M = 640 is 2.5 tiles of 256 and 5 of 128; N = 384 is 1.5 tiles of 256; K = 64 / 96 are 2 / 3 k-tiles; K = 512 is the
shortest contraction the planner may split."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M = 640
EPI_NONE, EPI_GELU, EPI_MUL_DGELU = 0, 1, 3
# every form a listed launch can take: 128x128, 256x256, and 128x128 with split-K (plain epilogues only, as for the unlisted launch)
FORMS = [
    pytest.param({"GEMM_TILE": 0, "GEMM_SPLITS": 1}, (128, 1), id="128x128"),
    pytest.param({"GEMM_TILE": 4, "GEMM_SPLITS": 1}, (256, 1), id="256x256"),
]
LISTS = ("none", "all", "count1", "count127", "count128", "count129", "count255", "count256", "count257", "half", "frames")
EPILOGUES = ("bias", "gelu", "dgelu", "beta1")


def _masks(rng):
    out = {"none": np.zeros(M, bool), "all": np.ones(M, bool)}
    for c in (1, 127, 128, 129, 255, 256, 257):
        m = np.zeros(M, bool)
        m[rng.choice(M, c, replace=False)] = True
        out[f"count{c}"] = m
    out["half"] = rng.random(M) < 0.5
    m = np.zeros(M, bool)          # frame-shaped runs, as synth.make_batch pads: per item a valid prefix of whole frames
    L = M // 8
    for b in range(8):
        m[b * L: b * L + (L // 8) * int(rng.integers(3, 9))] = True
    out["frames"] = m
    return out


_CACHE = {}


def _operands(dev, N, K, transB):
    """Per shape, made once and left unchanged."""
    key = (N, K, transB)
    if key not in _CACHE:
        g = torch.Generator(device="cpu").manual_seed(N * 3 + K * 5 + transB)
        _CACHE[key] = dict(A=torch.randn(M, K, generator=g).to(dev), B=torch.randn((N, K) if transB else (K, N), generator=g).to(dev),
                           bias=torch.randn(N, generator=g).to(dev), aux=torch.randn(M, N, generator=g).to(dev),
                           S=torch.randn(M, N, generator=g).to(dev), masks=_masks(np.random.default_rng(N + K)))
    return _CACHE[key]


def _launch(dev, A, B, transB, N, K, epi, C, aux=None, bias=None, beta=0.0, perm=None, count=None, hint=0, flags=0, rows=None):
    """One launch through the C ABI: ytvln_gemm_f32_rows when a list is given, ytvln_gemm_f32 otherwise.  C (and aux) are written in place.
    `rows` = the M of the launch when it is not the module's."""
    from ytvln import _lib
    from ytvln.ops import _ptr, _stream
    lib = _lib.load()
    M = rows or globals()["M"]
    ldb = K if transB else N
    if perm is None:
        need = int(lib.ytvln_gemm_workspace_elems(M, N, K, epi))
        ws = torch.empty(max(need, 1), device=dev)
        _lib.call("ytvln_gemm_f32", _ptr(A), K, 0, _ptr(B), ldb, int(transB), _ptr(C), N, _ptr(bias), _ptr(aux), N, M, N, K, epi, float(beta),
                  _ptr(ws), need, flags, _stream())
    else:
        need = int(lib.ytvln_gemm_rows_workspace_elems(M, N, K, epi, hint))
        ws = torch.empty(max(need, 1), device=dev)
        _lib.call("ytvln_gemm_f32_rows", _ptr(A), K, 0, _ptr(B), ldb, int(transB), _ptr(C), N, _ptr(bias), _ptr(aux), N, M, N, K, epi, float(beta),
                  _ptr(ws), need, flags, perm.data_ptr(), count.data_ptr(), int(hint), _stream())
    return C


def _case(dev, o, transB, N, K, kind, mt=None, lr=None, hint=0):
    """-> (C, aux written or None).  mt = None: the unlisted launch on the finite operands; else the listed launch on the poisoned ones."""
    nan = torch.full((), float("nan"), device=dev)
    A = o["A"] if mt is None else torch.where(mt[:, None], o["A"], nan)
    kw = {} if lr is None else dict(perm=lr.perm, count=lr.count, hint=hint)
    if kind == "bias":
        return _launch(dev, A, o["B"], transB, N, K, EPI_NONE, torch.full((M, N), float("nan"), device=dev), bias=o["bias"], **kw), None
    if kind == "gelu":
        z = torch.full((M, N), float("nan"), device=dev)
        return _launch(dev, A, o["B"], transB, N, K, EPI_GELU, torch.full((M, N), float("nan"), device=dev), aux=z, bias=o["bias"], **kw), z
    if kind == "dgelu":
        x = o["aux"] if mt is None else torch.where(mt[:, None], o["aux"], nan)
        return _launch(dev, A, o["B"], transB, N, K, EPI_MUL_DGELU, torch.full((M, N), float("nan"), device=dev), aux=x, **kw), None
    assert kind == "beta1"
    return _launch(dev, A, o["B"], transB, N, K, EPI_NONE, o["S"].clone(), beta=1.0, **kw), None


def _rows_plan(lib, N, K, epi, hint):
    tm, tn, sp = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.ytvln_gemm_rows_plan(M, N, K, epi, hint, ctypes.byref(tm), ctypes.byref(tn), ctypes.byref(sp)) == 0
    return tm.value, tn.value, sp.value


def _check(dev, lib, N, K, transB, force, want_plan, kinds):
    from ytvln import _lib, ops
    prev = {k: _lib.set_option(k, v) for k, v in force.items()}
    try:
        o = _operands(dev, N, K, transB)
        for kind in kinds:
            epi = {"bias": EPI_NONE, "gelu": EPI_GELU, "dgelu": EPI_MUL_DGELU, "beta1": EPI_NONE}[kind]
            tm, tn, sp = _rows_plan(lib, N, K, epi, 0)
            assert (tm, tn) == (want_plan[0],) * 2 and sp == want_plan[1], (tm, tn, sp)
            ref_c, ref_x = _case(dev, o, transB, N, K, kind)
            assert bool(torch.isfinite(ref_c).all())
            for name in LISTS:
                mask = o["masks"][name]
                mt = torch.from_numpy(mask).to(dev)
                lr = ops.live_rows(mt, perm=True)
                count = int(mask.sum())
                # the new list entry point against its numpy statement: live ascending, dead ascending, count
                assert int(lr.count.item()) == count
                assert np.array_equal(lr.perm.cpu().numpy(), np.concatenate([np.flatnonzero(mask), np.flatnonzero(~mask)]).astype(np.int32))
                c, x = _case(dev, o, transB, N, K, kind, mt, lr, hint=0)
                tag = (N, K, transB, kind, name)
                assert bool(torch.isfinite(c).all()), tag
                assert torch.equal(c[mt], ref_c[mt]), ("listed rows differ from the unlisted launch", tag)
                if kind == "beta1":
                    assert torch.equal(c[~mt], o["S"][~mt]), ("dead rows touched", tag)
                else:
                    assert int((c[~mt] != 0).sum()) == 0, ("dead rows not zero", tag)
                if x is not None:
                    assert bool(torch.isfinite(x).all()), tag
                    assert torch.equal(x[mt], ref_x[mt]) and int((x[~mt] != 0).sum()) == 0, ("aux", tag)
                # a second launch, and the hints: too small, exact, too large, none -- the same bits wherever the plan keeps the split count
                for hint in (0, count // 2, count, M):
                    if _rows_plan(lib, N, K, epi, hint)[2] != sp:
                        continue
                    c2, x2 = _case(dev, o, transB, N, K, kind, mt, lr, hint=hint)
                    assert torch.equal(c2, c), ("hint", hint, tag)
                    assert x is None or torch.equal(x2, x), ("hint aux", hint, tag)
    finally:
        for k, v in prev.items():
            _lib.set_option(k, v)


@pytest.mark.parametrize("force,want_plan", FORMS)
@pytest.mark.parametrize("transB", (1, 0), ids=("B=NxK", "B=KxN"))
@pytest.mark.parametrize("K", (64, 96))
@pytest.mark.parametrize("N", (256, 384))
def test_listed_launch_against_the_unlisted_one_on_the_same_plan(dev, lib, N, K, transB, force, want_plan):
    _check(dev, lib, N, K, transB, force, want_plan, EPILOGUES)


@pytest.mark.parametrize("transB", (1, 0), ids=("B=NxK", "B=KxN"))
@pytest.mark.parametrize("N", (256, 384))
def test_listed_split_k_launch(dev, lib, N, transB):
    """Split-K (plain epilogues): partials by list position, list-aware reduce."""
    _check(dev, lib, N, 512, transB, {"GEMM_TILE": 0, "GEMM_SPLITS": 2}, (128, 2), ("bias", "beta1"))


def test_ops_gemm_passes_the_list_unless_the_hint_is_the_row_count(dev, lib):
    from ytvln import ops
    N, K = 256, 64
    o = _operands(dev, N, K, 1)
    mask = o["masks"]["half"]
    mt = torch.from_numpy(mask).to(dev)
    A = torch.where(mt[:, None], o["A"], torch.full((), float("nan"), device=dev))
    lr = ops.live_rows(mt, perm=True)
    ref = torch.empty(M, N, device=dev)
    ops._gemm(o["A"], K, 0, o["B"], K, 1, ref, N, M, N, K, bias=o["bias"])
    for hint in (0, 256, 512):
        lr.hint = hint
        c = torch.full((M, N), float("nan"), device=dev)
        ops._gemm(A, K, 0, o["B"], K, 1, c, N, M, N, K, bias=o["bias"], rows=lr)
        assert torch.equal(c[mt], ref[mt]) and int((c[~mt] != 0).sum()) == 0, hint
    lr.hint = M          # "every row is expected": the plain launch, which reads the poisoned rows
    c = torch.empty(M, N, device=dev)
    ops._gemm(A, K, 0, o["B"], K, 1, c, N, M, N, K, bias=o["bias"], rows=lr)
    assert torch.equal(c[mt], ref[mt]) and bool(torch.isnan(c[~mt]).all())


def test_option_off_and_ineligible_launches_ignore_the_list(dev, lib):
    """GEMM_LIVE_M = 0, K % 32 != 0 (the launch leaves the LDS-DMA loop) and fp32x3: the list is ignored and the result is the unlisted
    launch's, bit for bit -- with a list that names NO row, which a launch that read it would answer with zeros."""
    from ytvln import _lib, ops
    g = torch.Generator(device="cpu").manual_seed(9)
    N = 256
    lr = ops.live_rows(torch.zeros(M, dtype=torch.bool, device=dev), perm=True)
    assert int(lr.count.item()) == 0
    for K, opt, flags in ((64, 0, 0), (80, 1, 0), (64, 1, _lib.GEMM_SPLIT_BF16X3)):
        A = torch.randn(M, K, generator=g).to(dev)
        B = torch.randn(N, K, generator=g).to(dev)
        prev = _lib.set_option("GEMM_LIVE_M", opt)
        try:
            plain = _launch(dev, A, B, 1, N, K, EPI_NONE, torch.empty(M, N, device=dev), flags=flags)
            listed = _launch(dev, A, B, 1, N, K, EPI_NONE, torch.empty(M, N, device=dev), perm=lr.perm, count=lr.count, flags=flags)
        finally:
            _lib.set_option("GEMM_LIVE_M", prev)
        assert torch.equal(plain, listed), (K, opt, flags)
        assert float(listed.abs().max()) > 0.0


def test_split_launch_that_cannot_be_reduced_by_list_stays_unlisted(dev, lib):
    """B = [N, K] may have any N; the list-aware reduce works in 16-byte pieces of a row.  N = 258 with a contraction the planner splits: the
    launch must ignore the list and return the unlisted launch's bits on EVERY row, also with a list that names no row."""
    import ctypes
    from ytvln import ops
    N, K = 258, 4096
    tm, tn, sp = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.ytvln_gemm_rows_plan(M, N, K, EPI_NONE, 0, ctypes.byref(tm), ctypes.byref(tn), ctypes.byref(sp)) == 0
    assert sp.value > 1, sp.value
    g = torch.Generator(device="cpu").manual_seed(21)
    A, B, bias = torch.randn(M, K, generator=g).to(dev), torch.randn(N, K, generator=g).to(dev), torch.randn(N, generator=g).to(dev)
    plain = _launch(dev, A, B, 1, N, K, EPI_NONE, torch.full((M, N), float("nan"), device=dev), bias=bias)
    assert bool(torch.isfinite(plain).all())
    for mask in (torch.zeros(M, dtype=torch.bool, device=dev), torch.rand(M, generator=torch.Generator().manual_seed(3)).to(dev) < 0.5):
        lr = ops.live_rows(mask, perm=True)
        for hint in (0, 256):
            listed = _launch(dev, A, B, 1, N, K, EPI_NONE, torch.full((M, N), float("nan"), device=dev), bias=bias, perm=lr.perm, count=lr.count,
                             hint=hint)
            assert torch.equal(listed, plain), (int(mask.sum()), hint)
    # the same contraction with N % 4 == 0 is listed (and split): dead rows are zeros
    N2 = 256
    assert lib.ytvln_gemm_rows_plan(M, N2, K, EPI_NONE, 0, ctypes.byref(tm), ctypes.byref(tn), ctypes.byref(sp)) == 0 and sp.value > 1
    B2 = B[:N2].contiguous()
    plain2 = _launch(dev, A, B2, 1, N2, K, EPI_NONE, torch.empty(M, N2, device=dev))
    lr = ops.live_rows(mask, perm=True)
    listed2 = _launch(dev, torch.where(mask[:, None], A, torch.full((), float("nan"), device=dev)), B2, 1, N2, K, EPI_NONE,
                      torch.full((M, N2), float("nan"), device=dev), perm=lr.perm, count=lr.count)
    assert torch.equal(listed2[mask], plain2[mask]) and int((listed2[~mask] != 0).sum()) == 0


def test_the_tile_the_hint_picks_does_not_change_the_bits(dev, lib):
    """Nothing forced: at 16128 x 1024 x 1024 the planner takes one round of 256x256 tiles for the full M and two rounds of 128x128 for a hint
    of 8192 rows (asserted).  Listed rows carry the bits of the unlisted launch under either tile, both B layouts."""
    import ctypes
    from ytvln import ops
    Mb, N, K = 16128, 1024, 1024
    tiles = {}
    for hint in (0, 8192):
        tm, tn, sp = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert lib.ytvln_gemm_rows_plan(Mb, N, K, EPI_NONE, hint, ctypes.byref(tm), ctypes.byref(tn), ctypes.byref(sp)) == 0
        tiles[hint] = (tm.value, sp.value)
    assert tiles[0][0] == 256 and tiles[8192][0] == 128 and tiles[0][1] == tiles[8192][1], tiles
    g = torch.Generator(device="cpu").manual_seed(31)
    A0 = torch.randn(Mb, K, generator=g).to(dev)
    mask = (torch.rand(Mb, generator=g) < 0.5).to(dev)
    A = torch.where(mask[:, None], A0, torch.full((), float("nan"), device=dev))
    lr = ops.live_rows(mask, perm=True)
    for transB in (1, 0):
        B = torch.randn((N, K) if transB else (K, N), generator=g).to(dev)
        plain = _launch(dev, A0, B, transB, N, K, EPI_NONE, torch.empty(Mb, N, device=dev), rows=Mb)
        for hint in (0, 8192):
            c = _launch(dev, A, B, transB, N, K, EPI_NONE, torch.full((Mb, N), float("nan"), device=dev), perm=lr.perm, count=lr.count, hint=hint,
                        rows=Mb)
            assert torch.equal(c[mask], plain[mask]), (transB, hint)
            assert int((c[~mask] != 0).sum()) == 0, (transB, hint)
