#!/usr/bin/env python
"""Weight-gradient GEMMs over the valid rows only, per cfg-2 shape: the unlisted launch, the identity list and the bench batch's list.

Protocol of profiles/README.md: every pass starts behind 0.4 s of GEMM, the three configurations are interleaved, the order is reversed
every pass, min of three passes.  Identity against unlisted = the cost of indexing; (identity - bench list) / (tiles saved) = the loop's
slope per k-tile.  Writes profiles/wgrad_live_rows_cost.json."""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "youtube-vln_amd"))
from ytvln import _lib, ops, synth  # noqa: E402

# (out, in, rows): the dW shapes of cfg 2 -- image side over 16128 rows, text side over 4480
SHAPES = [(1024, 1024, 16128), (2048, 1024, 16128), (1024, 2048, 16128), (1024, 4096, 16128), (4096, 1024, 16128), (1024, 12, 16128),
          (768, 768, 4480), (2304, 768, 4480), (768, 3072, 4480), (3072, 768, 4480), (1024, 768, 4480), (30524, 768, 4480)]
REPS = 10


def warm(dev, seconds=0.4):
    a = torch.randn(4096, 4096, device=dev)
    t = time.perf_counter()
    while time.perf_counter() - t < seconds:
        a @ a
    torch.cuda.synchronize()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / REPS


def main():
    dev = torch.device("cuda", 0)
    nb = synth.make_batch(bs=8, K=7, T=80, frames=8, boxes=36)          # the bench batch (seed 1234)
    masks = {4480: torch.from_numpy(np.asarray(nb[7]).reshape(-1) != 0).to(dev), 16128: torch.from_numpy(np.asarray(nb[3]).reshape(-1) > 0).to(dev)}
    out = {"protocol": "0.4 s of GEMM first, interleaved, order reversed every pass, min of 3; us per launch (GEMM + split-K reduce)", "shapes": []}
    for M, N, K in SHAPES:
        tm, tn, sp = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.load().ytvln_gemm_plan(M, N, K, 1, 0, ctypes.byref(tm), ctypes.byref(tn), ctypes.byref(sp))
        mask = masks[K]
        A = torch.randn(K, M, device=dev) * mask[:, None]
        B = torch.randn(K, N, device=dev)
        C = torch.empty(M, N, device=dev)
        db = torch.empty(M, device=dev)
        lists = {"unlisted": None, "identity": ops.live_rows(torch.ones(K, dtype=torch.bool, device=dev)), "bench": ops.live_rows(mask)}
        best = {k: float("inf") for k in lists}
        spread = {k: [] for k in lists}
        for p in range(3):
            warm(dev)
            order = list(lists) if p % 2 == 0 else list(lists)[::-1]
            for k in order:
                t = timed(lambda: ops._gemm(A, M, 1, B, N, 0, C, N, M, N, K, rowsum=db, live=lists[k]))
                best[k] = min(best[k], t)
                spread[k].append(t)
        live = int(mask.sum())
        tiles, live_tiles = K // 32, -(-live // 32)
        rec = {"M": M, "N": N, "K": K, "tile": [tm.value, tn.value], "splits": sp.value, "live_rows": live, "k_tiles": tiles, "live_k_tiles": live_tiles,
               "us": {k: round(v, 2) for k, v in best.items()}, "passes_us": {k: [round(x, 2) for x in v] for k, v in spread.items()},
               "unlisted_spread_us": round(max(spread["unlisted"]) - min(spread["unlisted"]), 2),
               "indexing_cost_us": round(best["identity"] - best["unlisted"], 2),
               "slope_us_per_k_tile_per_split": round((best["identity"] - best["bench"]) / max(1, -(-tiles // sp.value) - -(-live_tiles // sp.value)), 3)}
        out["shapes"].append(rec)
        print(json.dumps(rec), file=sys.stderr)
    path = os.path.join(ROOT, "profiles", "wgrad_live_rows_cost.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(path)


if __name__ == "__main__":
    main()
