"""CPU: the ABI of the bias-gradient launch (ytvln_attn_dbias_*: argument checks that fail before anything is enqueued, the workspace-size
function and its run plan) and the Python route from a bias that requires grad to that call -- the records it builds for the n1 / nh / 11,
transposed and expanded cases.  No GPU is touched: bad records are rejected on the host, and the route is followed with `ops.call` stubbed."""
import ctypes

import pytest
import torch

NEW = ("ytvln_attn_dbias_chunks", "ytvln_attn_dbias_workspace_elems", "ytvln_attn_dbias_f32", "ytvln_attn_dbias_bf16")


def _rec(ptr=64, sn=0, sh=0, sq=0, sk=1):
    from ytvln import _lib
    r = _lib.AttnBias()
    r.ptr, r.stride_n, r.stride_h, r.stride_q, r.stride_k = ptr, sn, sh, sq, sk
    return r


def _problem(Tq=4, Tk=4, p=0.0):
    """a record whose pointers are non-NULL and 16-byte aligned (never dereferenced: every call below is rejected on the host)"""
    from ytvln import _lib
    pr = _lib.AttnProblem()
    pr.q = pr.k = pr.v = pr.dctx = pr.lse_in = pr.delta = 256
    pr.ldq = pr.ldk = pr.ldv = pr.ldo = 64
    pr.Tq, pr.Tk, pr.p_drop = Tq, Tk, p
    return pr


def test_binding_and_abi_version_are_additive():
    import __graft_entry__ as g
    g.build()
    from ytvln import _lib
    lib = _lib.load()
    launch = [ctypes.c_void_p] * 4 + [ctypes.c_int64] + [ctypes.c_int] * 3 + [ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.SIGNATURES["ytvln_attn_dbias_f32"] == _lib.SIGNATURES["ytvln_attn_dbias_bf16"] == launch
    assert _lib.RESTYPES["ytvln_attn_dbias_workspace_elems"] is ctypes.c_int64
    assert lib.ytvln_version() == _lib.ABI_VERSION == 2
    assert lib.ytvln_attn_problem_size() == ctypes.sizeof(_lib.AttnProblem) == 192 and lib.ytvln_attn_bias_size() == 40


@pytest.mark.parametrize("name,d", [("ytvln_attn_dbias_f32", 64), ("ytvln_attn_dbias_bf16", 64)])
def test_bad_records_are_rejected_before_anything_is_enqueued(name, d):
    from ytvln import _lib
    lib = _lib.load()
    fn = getattr(lib, name)
    pr, out = _problem(), _rec(sq=4)
    A = ctypes.addressof

    def rejected(msg, p=pr, bias=None, o=out, ws=None, wse=0, N=1, heads=1, d_=d, rng=None):
        rc = fn(A(p) if p is not None else None, A(bias) if bias is not None else None, A(o) if o is not None else None, ws, wse, N, heads, d_,
                0.125, rng, None)
        assert rc < 0 and msg in lib.ytvln_last_error(), (rc, lib.ytvln_last_error())

    rejected(b"null problem", p=None)
    rejected(b"null output", o=None)
    rejected(b"null output", o=_rec(ptr=0, sq=4))                       # a record without a pointer
    rejected(b"positive", N=0)
    rejected(b"4-byte aligned", o=_rec(ptr=66, sq=4))                   # misaligned output
    rejected(b"non-negative", o=_rec(sq=-4))                            # negative stride
    rejected(b"non-negative", o=_rec(sq=4, sk=-1))
    rejected(b"2^31", o=_rec(sq=1 << 31))                               # plane offsets must stay 32-bit
    rejected(b"4-byte aligned", bias=_rec(ptr=70, sq=4))                # the forward bias is checked like the bias operand of the forward
    rejected(b"non-negative", bias=_rec(sq=-4))
    rejected(b"2^31", bias=_rec(sq=1 << 31))
    rejected(b"head dim", d_=36 if name.endswith("bf16") else 6)
    rejected(b"head dim", d_=256)
    bad = _problem()
    bad.q = 260
    rejected(b"16-byte aligned", p=bad)
    bad = _problem()
    bad.delta = None
    rejected(b"null pointer", p=bad)
    bad = _problem()
    bad.ldk = 66
    rejected(b"leading dimensions", p=bad)
    rejected(b"dropout needs", p=_problem(p=0.1))                        # fp32: no rng record; bf16: no keep buffer
    rejected(b"p_drop out of range", p=_problem(p=1.0))
    # a [1,1,Tq,Tk] output over 64 x 12 problems needs a workspace: absent, short, misaligned
    big, o11 = _problem(Tq=80, Tk=80), _rec(sq=80)
    need = lib.ytvln_attn_dbias_workspace_elems(A(o11), 64, 12, 80, 80)
    assert need > 0
    rejected(b"workspace too small", p=big, o=o11, N=64, heads=12)
    rejected(b"workspace too small", p=big, o=o11, ws=256, wse=need - 1, N=64, heads=12)
    rejected(b"workspace must be 4-byte aligned", p=big, o=o11, ws=258, wse=need, N=64, heads=12)


def test_workspace_size_and_run_plan():
    """One run (no workspace) whenever at most 16 problems are summed; otherwise runs of equal length, at least 4 problems each, enough of them
    to bring the launch to 1024 waves -- a function of the shapes alone."""
    from ytvln import _lib
    lib = _lib.load()
    A = ctypes.addressof
    chunks, elems = lib.ytvln_attn_dbias_chunks, lib.ytvln_attn_dbias_workspace_elems
    nh, n1, o11 = _rec(sn=8 * 80 * 288, sh=80 * 288, sq=288), _rec(sn=80 * 288, sq=288), _rec(sq=288)
    for o in (nh, n1):
        assert chunks(A(o), 56, 8, 80, 288) == 1 and elems(A(o), 56, 8, 80, 288) == 0
    # [1,1,80,288]: 448 problems, 3 x 9 blocks of scores -> ceil(1024 / 27) = 38 runs wanted, run length ceil(448 / 38) = 12 -> 38 runs
    assert chunks(A(o11), 56, 8, 80, 288) == 38
    assert elems(A(o11), 56, 8, 80, 288) == 38 * 80 * 288
    # [N,1,..] over 32 heads: 32 problems per plane; 2 planes x 1 block -> capped at 4 problems per run: 8 runs
    assert chunks(A(_rec(sn=36, sq=6)), 2, 32, 6, 6) == 8 and elems(A(_rec(sn=36, sq=6)), 2, 32, 6, 6) == 8 * 2 * 36
    # a large launch needs no split however long the sum
    assert chunks(A(_rec(sn=576 * 576, sq=576)), 8, 32, 576, 576) == 1
    # 17 problems, one block: ceil(17 / 4) = 5 runs wanted, run length ceil(17 / 5) = 4 -> runs of 4, 4, 4, 4, 1
    assert chunks(A(o11), 1, 17, 8, 8) == 5 and elems(A(_rec(sq=8)), 1, 17, 8, 8) == 5 * 64
    assert chunks(None, 1, 1, 8, 8) < 0 and elems(A(o11), 0, 1, 8, 8) < 0


def _route(monkeypatch, bias, N, heads, Tq, Tk, fwd_bias=True, bf16=False):
    """ops._attn_dbias on CPU tensors with the launch stubbed: -> (entry point name, forward-bias record or None, output record, workspace
    elements, the returned gradient)."""
    from ytvln import _lib, ops
    seen = []

    def stub(name, *a):
        rec = lambda addr: None if addr is None else tuple(getattr(_lib.AttnBias.from_address(addr), f) for f, _ in _lib.AttnBias._fields_)  # noqa: E731
        seen.append((name, a[0], rec(a[1]), rec(a[2]), a[3], a[4], a[5:]))

    monkeypatch.setattr(ops, "call", stub)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    held, like = ops._trainable_bias(bias, True)
    assert held is not bias and not held.requires_grad and held.dtype == torch.float32 and like == (tuple(bias.shape), bias.dtype)
    pr = _lib.AttnProblem()
    g = ops._attn_dbias(pr, held if fwd_bias else None, like, bf16, N, heads, Tq, Tk, 64, 0.125, None, bias.device)
    (name, prp, brec, orec, ws, wse, rest), = seen
    assert prp == ctypes.addressof(pr) and rest[:4] == (N, heads, 64, 0.125)
    assert (ws is None) == (wse == 0)
    if brec is not None:
        assert brec[0] == held.data_ptr()
    assert orec[0] is not None and orec[0] != (brec[0] if brec else 0)          # a fresh buffer, never the bias itself
    return name, brec, orec, wse, g


def test_python_route_builds_the_right_records(monkeypatch):
    N, h, Tq, Tk = 3, 4, 5, 7
    # n1: summed over heads in the library (stride_h = 0), read and written as it lies
    name, b, o, wse, g = _route(monkeypatch, torch.zeros(N, 1, Tq, Tk, requires_grad=True), N, h, Tq, Tk)
    assert name == "ytvln_attn_dbias_f32" and b[1:] == o[1:] == (Tq * Tk, 0, Tk, 1) and wse == 0 and tuple(g.shape) == (N, 1, Tq, Tk)
    # nh
    name, b, o, wse, g = _route(monkeypatch, torch.zeros(N, h, Tq, Tk, requires_grad=True), N, h, Tq, Tk, bf16=True)
    assert name == "ytvln_attn_dbias_bf16" and b[1:] == o[1:] == (h * Tq * Tk, Tq * Tk, Tk, 1) and tuple(g.shape) == (N, h, Tq, Tk)
    # 11: both sums in the library
    _, b, o, wse, g = _route(monkeypatch, torch.zeros(1, 1, Tq, Tk, requires_grad=True), N, h, Tq, Tk)
    assert b[1:] == o[1:] == (0, 0, Tk, 1) and wse == 0 and tuple(g.shape) == (1, 1, Tq, Tk)
    # 11 over many problems: the workspace the library asks for is allocated and handed over
    _, b, o, wse, g = _route(monkeypatch, torch.zeros(1, 1, Tq, Tk, requires_grad=True), 40, h, Tq, Tk)
    assert wse == 40 * Tq * Tk                      # 160 problems, one block: 4 per run -> 40 runs
    # transposed view of an [N,1,Tk,Tq] leaf: the forward values are read through swapped strides, the gradient is that of the VIEW (contiguous)
    co = torch.zeros(N, 1, Tk, Tq, requires_grad=True)
    _, b, o, wse, g = _route(monkeypatch, co.transpose(2, 3), N, h, Tq, Tk)
    assert b[1:] == (Tq * Tk, 0, 1, Tq) and o[1:] == (Tq * Tk, 0, Tk, 1) and tuple(g.shape) == (N, 1, Tq, Tk)
    # expanded [1,h,Tq,Tk] -> [N,h,Tq,Tk]: read with stride_n = 0, but the gradient is the FULL [N,h,..] one (autograd's expand-backward sums it)
    par = torch.zeros(1, h, Tq, Tk, requires_grad=True)
    _, b, o, wse, g = _route(monkeypatch, par.expand(N, h, Tq, Tk), N, h, Tq, Tk)
    assert b[1:] == (0, Tq * Tk, Tk, 1) and o[1:] == (h * Tq * Tk, Tq * Tk, Tk, 1) and tuple(g.shape) == (N, h, Tq, Tk)
    # no forward bias record (layout of the gradient only)
    _, b, o, wse, g = _route(monkeypatch, torch.zeros(N, 1, Tq, Tk, requires_grad=True), N, h, Tq, Tk, fwd_bias=False)
    assert b is None and o[1:] == (Tq * Tk, 0, Tk, 1)
    # dtype round trip: fp32 inside, the bias's own dtype out
    for dt in (torch.bfloat16, torch.float64):
        _, b, o, wse, g = _route(monkeypatch, torch.zeros(N, 1, Tq, Tk, dtype=dt, requires_grad=True), N, h, Tq, Tk)
        assert g.dtype == dt and tuple(g.shape) == (N, 1, Tq, Tk)


def test_a_constant_bias_passes_through_untouched_and_the_raw_helper_still_refuses():
    from ytvln import ops
    b = torch.zeros(2, 1, 3, 3)
    assert ops._trainable_bias(b, False) == (b, None) and ops._trainable_bias(None, True) == (None, None)
    t = torch.zeros(2, 1, 3, 3, requires_grad=True)
    assert ops._trainable_bias(t, False)[0] is t                      # not asked for a gradient: handed on as it is
    with pytest.raises(RuntimeError, match="requires_grad"):
        ops._attn_bias(t, 2, 4, 3, 3)
