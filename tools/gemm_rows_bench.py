"""Row-listed fp32 GEMMs against the unlisted launches, per cfg-2 shape: forward (B = [N, K]), input gradient (B = [K, N]) and weight
gradient (A = dY^T).  Per shape: the unlisted launch; the identity list with m_hint = M (what a batch without padding would pay for carrying
a list); the list of a batch with the bench batch's share of valid rows (8031 of 16128 image rows, 2662 of 4480 text rows, a valid prefix per
item of 56 items) with its hint (the count rounded up to 256).  The protocol of tools/gemm_sk_bench.py: every pass starts behind 0.4 s of GEMM
(clocks), the variants are interleaved and the order is reversed every other pass, min and max over PASSES passes per variant (HIP events,
ITERS launches each).  Writes rows_gemm_shapes.json into OUT (default: the working directory).  SHAPES=fwd|dgrad|wgrad|all."""
import json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "youtube-vln_amd"))
import numpy as np
import torch
from ytvln import ops, _lib
from ytvln.ops import _ptr, _stream
dev = torch.device("cuda", 0)
lib = _lib.load()
LIVE = {16128: 8031, 4480: 2662}
ITEMS = 56
# (M, N, K, transB) of the encoder's projections; weight gradients as (M, N, K) with K the rows of the batch
FWD = [(16128, 1024, 1024, 1), (16128, 3072, 1024, 1), (16128, 1024, 2048, 1), (16128, 1024, 768, 1), (4480, 768, 768, 1), (4480, 2304, 768, 1),
       (4480, 3072, 768, 1), (4480, 768, 3072, 1), (4480, 1024, 768, 1), (4480, 768, 1024, 1), (4480, 2048, 768, 1)]
DGRAD = [(16128, 1024, 1024, 0), (16128, 1024, 3072, 0), (16128, 2048, 1024, 0), (4480, 768, 768, 0), (4480, 768, 2304, 0), (4480, 768, 3072, 0),
         (4480, 3072, 768, 0), (4480, 768, 1024, 0), (4480, 1024, 768, 0), (4480, 768, 2048, 0)]
WGRAD = [(1024, 1024, 16128), (3072, 1024, 16128), (2048, 1024, 16128), (1024, 3072, 16128), (768, 768, 4480), (768, 3072, 4480), (3072, 768, 4480),
         (2304, 768, 4480)]
which = os.environ.get("SHAPES", "all")
ITERS, PASSES = int(os.environ.get("ITERS", "20")), int(os.environ.get("PASSES", "3"))
hot_a, hot_b = torch.randn(8192, 8192, device=dev), torch.randn(8192, 8192, device=dev)


def heat(ms=400):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    while True:
        for _ in range(10): torch.mm(hot_a, hot_b)
        e1.record(); torch.cuda.synchronize()
        if e0.elapsed_time(e1) > ms: return


def timed(fn):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS * 1000


def batch_mask(rows):
    per, live = rows // ITEMS, LIVE[rows]
    m = np.zeros(rows, bool)
    for i in range(ITEMS):
        m[i * per: i * per + live // ITEMS + (1 if i < live % ITEMS else 0)] = True
    assert int(m.sum()) == live
    return torch.from_numpy(m).to(dev)


def measure(variants):
    best, worst = {}, {}
    for ps in range(PASSES):
        heat()
        for name, fn in (variants if ps % 2 == 0 else variants[::-1]):
            us = timed(fn)
            best[name], worst[name] = min(best.get(name, 1e30), us), max(worst.get(name, 0.0), us)
    return {n: {"us_min": round(best[n], 1), "us_max": round(worst[n], 1)} for n, _ in variants}


def rows_launch(A, B, tb, C, M, N, K, lr, hint):
    need = int(lib.ytvln_gemm_rows_workspace_elems(M, N, K, 0, hint))
    ws = torch.empty(max(need, 1), device=dev)
    return lambda: _lib.call("ytvln_gemm_f32_rows", _ptr(A), K, 0, _ptr(B), B.stride(0), tb, _ptr(C), N, None, None, 0, M, N, K, 0, 0.0, _ptr(ws), need, 0,
                             lr.perm.data_ptr(), lr.count.data_ptr(), hint, _stream())


out = []
if which in ("fwd", "dgrad", "all"):
    for kind, shapes in (("fwd", FWD), ("dgrad", DGRAD)):
        if which not in (kind, "all"):
            continue
        for (M, N, K, tb) in shapes:
            A, B, C = torch.randn(M, K, device=dev), torch.randn((N, K) if tb else (K, N), device=dev), torch.empty(M, N, device=dev)
            ident = ops.live_rows(torch.ones(M, dtype=torch.bool, device=dev), perm=True)
            part = ops.live_rows(batch_mask(M), perm=True)
            hint = -(-LIVE[M] // 256) * 256
            r = measure([("unlisted", lambda: ops._gemm(A, K, 0, B, B.stride(0), tb, C, N, M, N, K)),
                         ("identity_hint_M", rows_launch(A, B, tb, C, M, N, K, ident, M)),
                         ("batch_list", rows_launch(A, B, tb, C, M, N, K, part, hint))])
            rec = {"kind": kind, "M": M, "N": N, "K": K, "transB": tb, "live": LIVE[M], "hint": hint, **r}
            out.append(rec); print(json.dumps(rec), flush=True)
if which in ("wgrad", "all"):
    for (M, N, K) in WGRAD:
        part_m = batch_mask(K)
        A = torch.randn(K, M, device=dev) * part_m[:, None]          # dY: zero on the padded rows
        B, C = torch.randn(K, N, device=dev), torch.empty(M, N, device=dev)
        ident, part = ops.live_rows(torch.ones(K, dtype=torch.bool, device=dev)), ops.live_rows(part_m)
        r = measure([("unlisted", lambda: ops._gemm(A, M, 1, B, N, 0, C, N, M, N, K)),
                     ("identity_list", lambda: ops._gemm(A, M, 1, B, N, 0, C, N, M, N, K, live=ident)),
                     ("batch_list", lambda: ops._gemm(A, M, 1, B, N, 0, C, N, M, N, K, live=part))])
        rec = {"kind": "wgrad", "M": M, "N": N, "K": K, "live": LIVE[K], **r}
        out.append(rec); print(json.dumps(rec), flush=True)
OUT = os.environ.get("OUT", ".")
os.makedirs(OUT, exist_ok=True)
json.dump({"what": __doc__.split("  Writes")[0], "iters": ITERS, "passes": PASSES, "shapes": out}, open(os.path.join(OUT, "rows_gemm_shapes.json"), "w"), indent=1)
