"""The stored-dS attention backward (attention.hip: attn_bwd_delta_body, attn_bwd_dkv_w1_body<STORE>, attn_bwd_dq_ds_body; option ATTN_W1 bit 3)
against the recomputing one-wave kernels it replaces (ATTN_W1 = 7).

The dK/dV wave writes each 32x32 block of dS it forms to a workspace and the dQ kernel only contracts those blocks with K, in the key-tile
order of attn_bwd_dq_w1_body; delta comes from a pass of its own with the arithmetic of that kernel's prologue.  So nothing may move: dq, dk, dv
and delta are compared with np.array_equal / torch.equal, never with a tolerance.  The fp64 comparison of the pair entry point uses the bounds of
tests/test_kernels_gpu.py::test_attention_fwd_bwd (rel-L2 2e-5 on rows that are not fully masked, 5e-3 on fully masked ones)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from helpers import rel_l2
from test_kernels_gpu import ref_attention, rnd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

_RUNS = {}


def _run(**options):
    """tools/attn_form_check.run (17 shapes, forward + backward) under the given options; one run per setting and session, never modified"""
    import attn_form_check as F
    key = tuple(sorted(options.items()))
    if key not in _RUNS:
        _RUNS[key] = F.run(options, True)
    return _RUNS[key]


def _options(**options):
    from ytvln import _lib
    prev = {k: _lib.set_option(k, v) for k, v in options.items()}
    return lambda: [_lib.set_option(k, v) for k, v in prev.items()]


def _elems(lib, N, heads, d, Tq, Tk, Tq_b=0, Tk_b=0):
    return int(lib.ytvln_attn_bwd_workspace_elems(N, heads, d, Tq, Tk, Tq_b, Tk_b))


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), (key, int((a[key] != b[key]).sum()), a[key].size)


def test_bit_identical_to_the_recomputing_kernels_at_every_shape(dev, lib):
    """ATTN_W1_DKV_ANY = 1: every launch of an unpadded d = 128 / 64 head with sequences up to 512 takes the stored form, the rest (d = 96, 68,
    576 keys) falls back silently."""
    import attn_form_check as F
    restore = _options(ATTN_W1=15, ATTN_W1_DKV_ANY=1)
    try:          # the shapes this comparison is about do take the form, the fall-back shapes do not
        taken = [_elems(lib, N, h, d, Tq, Tk) > 0 for N, h, d, Tq, Tk, _, _ in F.SHAPES]
        assert taken == [d in (64, 128) and max(Tq, Tk) <= 512 for _, _, d, Tq, Tk, _, _ in F.SHAPES] and sum(taken) == 14
    finally:
        restore()
    _assert_same(_run(ATTN_W1=7, ATTN_W1_DKV_ANY=1), _run(ATTN_W1=15, ATTN_W1_DKV_ANY=1))


def test_bit_identical_under_the_default_dkv_selection(dev, lib):
    """Without ATTN_W1_DKV_ANY the fill rule decides, and it sends every launch of these sizes to the wave-pair dK/dV kernel: bit 3 set changes
    nothing (test_missing_or_short_workspace_... hands such a launch a workspace all the same)."""
    import attn_form_check as F
    restore = _options(ATTN_W1=15, ATTN_W1_DKV_ANY=0)
    try:
        assert not any(_elems(lib, N, h, d, Tq, Tk) for N, h, d, Tq, Tk, _, _ in F.SHAPES)
        assert _elems(lib, 56, 8, 128, 288, 288) > 0          # (the training step's launches are large enough)
    finally:
        restore()
    _assert_same(_run(ATTN_W1=7), _run(ATTN_W1=15))


def _pair_problem(dev, N, heads, d, Tq, Tk, seed):
    """both directions of a co-attention site: problem a = Tq queries over Tk keys, problem b = Tk queries over Tq keys"""
    H = heads * d
    t = {"qa": rnd(dev, N * Tq, H, seed=seed), "kva": rnd(dev, N * Tk, 2 * H, seed=seed + 1), "qb": rnd(dev, N * Tk, H, seed=seed + 2),
         "kvb": rnd(dev, N * Tq, 2 * H, seed=seed + 3), "da": rnd(dev, N * Tq, H, seed=seed + 4), "db": rnd(dev, N * Tk, H, seed=seed + 5)}
    ma, mb = torch.zeros(N, Tk, device=dev), torch.zeros(N, Tq, device=dev)
    ma[0, Tk - max(1, Tk // 4):] = -10000.0
    mb[1, Tq - 5:] = -10000.0
    return t, ma, mb


def _keep_mask(dev, ops, st, site, N, heads, d, Tq, Tk, p):
    """the dropout decisions of a site, [N, heads, Tq, Tk]: q = k = 0 gives uniform probabilities, identity columns in v show which survived --
    d keys per forward launch (test_kernels_gpu.py::test_attention_dropout, in chunks)"""
    H = heads * d
    z, zk, out = torch.zeros(N * Tq, H, device=dev), torch.zeros(N * Tk, H, device=dev), torch.empty(N * Tq, H, device=dev)
    keep = torch.zeros(N, heads, Tq, Tk, dtype=torch.float64, device=dev)
    for c0 in range(0, Tk, d):
        eye = torch.zeros(N, Tk, heads, d, device=dev)
        for j in range(c0, min(c0 + d, Tk)):
            eye[:, j, :, j - c0] = 1.0
        ops._attn_fwd(z, 0, H, zk, 0, H, eye.reshape(N * Tk, H), 0, H, None, out, N, heads, Tq, Tk, d, 1 / math.sqrt(d), p, st.tensor, site)
        n = min(d, Tk - c0)
        keep[..., c0:c0 + n] = (out.view(N, Tq, heads, d)[..., :n] > 0).permute(0, 2, 1, 3).double()
    return keep


@pytest.mark.parametrize("Tq,Tk", [(80, 288), (37, 101)])
def test_pair_entry_point(dev, lib, Tq, Tk):
    """ytvln_attn_bwd_pair_ws: both directions in one launch per kernel, with dropout and masked keys -- bit-equal to ATTN_W1 = 7 and inside the
    fp64 bounds."""
    from ytvln import ops
    N, heads, d, p = 2, 2, 128, 0.1
    H, scale = heads * d, 1 / math.sqrt(d)
    t, ma, mb = _pair_problem(dev, N, heads, d, Tq, Tk, seed=11)
    st = ops.DropoutState(dev)
    sa, sb = 4, 5
    ca, cb = torch.empty_like(t["qa"]), torch.empty_like(t["qb"])
    la = torch.empty(N, heads, Tq, device=dev)
    lb = torch.empty(N, heads, Tk, device=dev)
    fa = ops._attn_problem(t["qa"], 0, H, t["kva"], 0, 2 * H, t["kva"], H, 2 * H, ma, Tq, Tk, p, sa, ctx=ca, lse=la)
    fb = ops._attn_problem(t["qb"], 0, H, t["kvb"], 0, 2 * H, t["kvb"], H, 2 * H, mb, Tk, Tq, p, sb, ctx=cb, lse=lb)
    ops._attn_launch(False, False, fa, fb, N, heads, d, scale, st.tensor)

    def backward(w1):
        restore = _options(ATTN_W1=w1, ATTN_W1_DKV_ANY=1)
        try:
            if w1 == 15:
                assert _elems(lib, N, heads, d, Tq, Tk, Tk, Tq) == 2 * N * heads * (32 * math.ceil(Tq / 32)) * (32 * math.ceil(Tk / 32))
            g = {"dqa": torch.zeros_like(t["qa"]), "dkva": torch.zeros_like(t["kva"]), "dqb": torch.zeros_like(t["qb"]),
                 "dkvb": torch.zeros_like(t["kvb"]), "delta_a": torch.zeros_like(la), "delta_b": torch.zeros_like(lb)}
            pa = ops._attn_problem(t["qa"], 0, H, t["kva"], 0, 2 * H, t["kva"], H, 2 * H, ma, Tq, Tk, p, sa, ctx_in=ca, dctx=t["da"], lse_in=la,
                                   delta=g["delta_a"], dq=g["dqa"], lddq=H, dk=g["dkva"], lddk=2 * H, dv=g["dkva"], dv_off=H, lddv=2 * H)
            pb = ops._attn_problem(t["qb"], 0, H, t["kvb"], 0, 2 * H, t["kvb"], H, 2 * H, mb, Tk, Tq, p, sb, ctx_in=cb, dctx=t["db"], lse_in=lb,
                                   delta=g["delta_b"], dq=g["dqb"], lddq=H, dk=g["dkvb"], lddk=2 * H, dv=g["dkvb"], dv_off=H, lddv=2 * H)
            ops._attn_launch(True, False, pa, pb, N, heads, d, scale, st.tensor)
            torch.cuda.synchronize()
            return g
        finally:
            restore()

    old, new = backward(7), backward(15)
    for key in old:
        assert torch.equal(old[key], new[key]), (key, int((old[key] != new[key]).sum()))
        assert float(new[key].abs().max()) > 0, key
    # fp64: each direction against the reference attention with this site's dropout decisions
    for q, kv, dout, mask, site, tq, tk, gq, gkv in ((t["qa"], t["kva"], t["da"], ma, sa, Tq, Tk, new["dqa"], new["dkva"]),
                                                     (t["qb"], t["kvb"], t["db"], mb, sb, Tk, Tq, new["dqb"], new["dkvb"])):
        keep = _keep_mask(dev, ops, st, site, N, heads, d, tq, tk, p)
        qd = q.double().view(N, tq, H).requires_grad_(True)
        kd = kv[:, :H].double().reshape(N, tk, H).requires_grad_(True)
        vd = kv[:, H:].double().reshape(N, tk, H).requires_grad_(True)
        ref, _ = ref_attention(qd, kd, vd, mask.double(), heads, keep, p)
        ref.backward(dout.double().view(N, tq, H))
        full = [n for n in range(N) if bool((mask[n] != 0).all())]
        part = [n for n in range(N) if n not in full]
        for rows, tol in ((part, 2e-5), (full, 5e-3)):
            if rows:
                assert rel_l2(gq.view(N, tq, H)[rows], qd.grad[rows]) < tol, "dq"
                assert rel_l2(gkv[:, :H].reshape(N, tk, H)[rows], kd.grad[rows]) < tol, "dk"
                assert rel_l2(gkv[:, H:].reshape(N, tk, H)[rows], vd.grad[rows]) < tol, "dv"


@pytest.mark.parametrize("d", [64, 128])
def test_graph_capture_replays_bit_equal(dev, lib, d):
    """Forward + backward of one self-attention site captured by torch.cuda.graph (the workspace is allocated inside the capture) and replayed
    twice: the gradients equal the eager ones bit for bit."""
    from ytvln import ops
    N, heads, T, p = 2, 2, 80, 0.1
    H = heads * d
    restore = _options(ATTN_W1=15, ATTN_W1_DKV_ANY=1)
    try:
        st = ops.DropoutState(dev)
        qkv = rnd(dev, N * T, 3 * H, seed=5).requires_grad_()
        mask = torch.zeros(N, T, device=dev)
        mask[0, T - 5:] = -10000.0
        dout = rnd(dev, N * T, H, seed=6)

        def step():
            out, _ = ops.SelfAttentionFn.apply(qkv, mask, N, T, heads, p, st.tensor, 9)
            return torch.autograd.grad(out, qkv, dout)[0]

        eager = step().clone()          # (st.tensor is this pass's frozen (seed, counter): eager and captured runs draw the same masks)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            captured = step()
        for _ in range(2):
            captured.zero_()
            gr.replay()
            torch.cuda.synchronize()
            assert torch.equal(captured, eager), float((captured - eager).abs().max())
        assert float(eager.abs().max()) > 0
    finally:
        restore()


def test_missing_or_short_workspace_takes_the_recomputing_path(dev, lib):
    """ytvln_attn_bwd_ws_f32 with NULL, with one float too few, with the whole workspace, and with a workspace for a launch that the fill rule
    sends to the wave-pair dK/dV kernel: no error, the same bits (all but the third run the recomputing kernels, as ytvln_attn_bwd_f32 does)."""
    from ytvln import _lib, ops
    N, heads, d, Tq, Tk = 2, 2, 128, 70, 45
    H, scale = heads * d, 1 / math.sqrt(d)
    q, k, v, dout = (rnd(dev, N * T, H, seed=s) for T, s in ((Tq, 1), (Tk, 2), (Tk, 3), (Tq, 4)))
    mask = torch.zeros(N, Tk, device=dev)
    mask[1, Tk - 7:] = -10000.0
    ctx = torch.empty_like(q)
    lse = ops._attn_fwd(q, 0, H, k, 0, H, v, 0, H, mask, ctx, N, heads, Tq, Tk, d, scale, 0.0, None, 0)
    restore = _options(ATTN_W1=15, ATTN_W1_DKV_ANY=1)
    try:
        need = _elems(lib, N, heads, d, Tq, Tk)
        assert need == N * heads * 96 * 64
        got = []
        for ws_elems, claimed, dkv_any in ((0, 0, 1), (need, need - 1, 1), (need, need, 1), (need, need, 0)):
            _lib.set_option("ATTN_W1_DKV_ANY", dkv_any)
            ws = torch.full((ws_elems,), float("nan"), device=dev) if ws_elems else None
            dq, dk, dv, delta = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v), torch.zeros_like(lse)
            _lib.call("ytvln_attn_bwd_ws_f32", q.data_ptr(), H, k.data_ptr(), H, v.data_ptr(), H, mask.data_ptr(), ctx.data_ptr(), dout.data_ptr(), H,
                      lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), H, dk.data_ptr(), H, dv.data_ptr(), H, N, heads, Tq, Tk, d, scale, 0.0, None, 0,
                      ws.data_ptr() if ws is not None else None, claimed, ops._stream())
            torch.cuda.synchronize()
            if ws is not None:          # a workspace the library declined stays untouched; the one it took holds whole blocks
                assert bool(torch.isnan(ws).all()) == (claimed < need or not dkv_any)
                assert dkv_any or _elems(lib, N, heads, d, Tq, Tk) == 0
            got.append((dq, dk, dv, delta))
        for other in got[1:]:
            for a, b, what in zip(got[0], other, ("dq", "dk", "dv", "delta")):
                assert torch.equal(a, b), what
        assert float(got[0][0].abs().max()) > 0
    finally:
        restore()
