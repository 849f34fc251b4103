#!/usr/bin/env python3
"""Cost of the EMA of the weights (AdamW.ema_decay) against the plain fused AdamW update on the full model's arena.

The full model of the bench's default workload (about 250 M parameters, every tensor given a random gradient so that all of them are in
the arena; no forward or backward pass is run), one optimizer, and two ways of launching its update over every launch class on the same
arenas in the same process: the plain update (one launch per class, 28 bytes per parameter) and the update followed by ytvln_ema_update
(two launches per class, 28 + 12 bytes per parameter).  Protocol of DESIGN.md section 5, shared with tools/grad_clip_cost.py and
tools/lamb_cost.py: every pass starts behind 0.4 s of GEMM (warm clocks), the configurations are interleaved, the order is reversed every
pass, min of the passes; a reading is the mean of `--reps` updates between two HIP events.  The EMA pass and the evaluation swap
(ytvln_ema_swap, 16 bytes per parameter) are also timed alone.  The yardstick of the EMA pass is the plain update's own rate in the same
run.  Writes profiles/ema_cost.json (or --out).

    python tools/ema_cost.py [--reps 20] [--passes 3] [--out profiles/ema_cost.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "youtube-vln_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from grad_clip_cost import PEAK_HBM_TBS, protocol  # noqa: E402
from lamb_cost import build  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_cost.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    from ytvln import ops
    model, opt = build(dev)
    arena = opt._arena
    elems = sum(numel for _, numel in arena["index"].values())
    opt.ema_decay = 0.999
    shadow = opt.ema_buffers()
    opt._upload_hyper()         # the EMA weight into slot 6 of every class's record
    torch.cuda.synchronize()

    def plain():
        opt.ema_decay = None
        opt.launch_classes()

    def with_ema():
        opt.ema_decay = 0.999
        opt.launch_classes()
    t = protocol(dev, {"adamw": plain, "adamw_ema": with_ema}, a.reps, a.passes)

    def ema_only():
        for c in opt._launch:
            ops.ema_update(arena["p"], shadow, c["table"], c["n"], c["hyper"], None)

    def swap_only():
        for c in opt._launch:
            ops.ema_swap(arena["p"], shadow, c["table"], c["n"], p_bf16=None)
    alone = protocol(dev, {"ema_update": ema_only, "ema_swap": swap_only}, a.reps, a.passes)
    torch.cuda.synchronize()
    res = {"model": "cfg2_full_pretrain_bs8", "parameters": elems, "arena_elements": int(arena["p"].numel()), "tensors": len(arena["index"]),
           "launch_classes": len(opt._launch), "records": sum(c["n"] for c in opt._launch), "reps_per_reading": a.reps, "passes": a.passes,
           "protocol": "0.4 s of GEMM before every pass, interleaved, order reversed every pass, min of the passes", "update_ms": {}}
    for name, nbytes in (("adamw", 28), ("adamw_ema", 40)):
        v = t[name]
        res["update_ms"][name] = {"min": min(v), "passes": v, "spread": max(v) - min(v), "bytes_per_parameter": nbytes,
                                  "tb_per_s": nbytes * elems / (min(v) * 1e-3) / 1e12}
    res["delta_ms_ema_minus_plain"] = res["update_ms"]["adamw_ema"]["min"] - res["update_ms"]["adamw"]["min"]
    res["ratio_ema_over_adamw"] = res["update_ms"]["adamw_ema"]["min"] / res["update_ms"]["adamw"]["min"]
    res["ratio_by_bytes"] = 40 / 28
    for name, nbytes in (("ema_update", 12), ("ema_swap", 16)):
        v = alone[name]
        rate = nbytes * elems / (min(v) * 1e-3) / 1e12
        res[name] = {"ms": min(v), "passes": v, "bytes_per_parameter": nbytes, "tb_per_s": rate,
                     "fraction_of_8_tb_per_s": rate / PEAK_HBM_TBS, "fraction_of_plain_update_rate": rate / res["update_ms"]["adamw"]["tb_per_s"]}
    res["parameters_finite"] = bool(torch.isfinite(arena["p"]).all()) and bool(torch.isfinite(shadow).all())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
