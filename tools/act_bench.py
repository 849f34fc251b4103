"""Achieved HBM bandwidth of the stand-alone activation kernels (csrc/norm.hip): ytvln_act_fwd_* (swish forward), the swish case of
ytvln_act_bwd_* and, as the yardstick with the same access pattern, the gelu case of ytvln_act_bwd_* -- same box, same run.

    python tools/act_bench.py [--iters 200] [--out FILE.json]

Bytes are the ones the algorithm needs (forward: one read + one write per element; backward: two reads + one write); time is device events
around `iters` back-to-back launches after a warm-up, best and median of five rounds.  The buffers (up to 200 MB per operand at fp32) do
not fit the 256 MiB last-level cache together, and each round walks a ring of four buffer sets so that no launch re-reads what the previous
one left there.  Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "youtube-vln_amd"))
from ytvln import _lib  # noqa: E402

SIZES = [(16128, 1024), (4480, 3072)]
RING = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "act_bench needs a HIP device"
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for rows_, cols in SIZES:
        n = rows_ * cols
        for dt, suffix, eb in ((torch.float32, "f32", 4), (torch.bfloat16, "bf16", 2)):
            sets = [tuple(torch.randn(n, device=dev).to(dt) for _ in range(2)) + (torch.empty(n, device=dev, dtype=dt),) for _ in range(RING)]
            cases = [("act_fwd swish", lambda z, d, o: _lib.call("ytvln_act_fwd_" + suffix, z.data_ptr(), o.data_ptr(), n, _lib.ACT_SWISH, st), 2),
                     ("act_bwd swish", lambda z, d, o: _lib.call("ytvln_act_bwd_" + suffix, d.data_ptr(), z.data_ptr(), o.data_ptr(), n, _lib.ACT_SWISH, st), 3),
                     ("act_bwd gelu", lambda z, d, o: _lib.call("ytvln_act_bwd_" + suffix, d.data_ptr(), z.data_ptr(), o.data_ptr(), n, _lib.EPI_GELU, st), 3)]
            for name, fn, streams in cases:
                for i in range(20):
                    fn(*sets[i % RING])
                torch.cuda.synchronize()
                times = []
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for i in range(a.iters):
                        fn(*sets[i % RING])
                    e1.record()
                    e1.synchronize()
                    times.append(e0.elapsed_time(e1) * 1e-3 / a.iters)
                nbytes = streams * n * eb
                r = dict(kernel=name, dtype=suffix, n=n, shape=[rows_, cols], bytes=nbytes, us_best=min(times) * 1e6,
                         us_median=statistics.median(times) * 1e6, gbps_best=nbytes / min(times) * 1e-9,
                         gbps_median=nbytes / statistics.median(times) * 1e-9)
                rows.append(r)
                print(f"{name:14s} {suffix:4s} n = {rows_} x {cols}: {r['us_median']:8.1f} us median ({r['us_best']:.1f} best)  "
                      f"{r['gbps_median']:7.0f} GB/s median ({r['gbps_best']:.0f} best)", flush=True)
            del sets
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
