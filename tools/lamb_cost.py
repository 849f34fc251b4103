#!/usr/bin/env python3
"""Cost of the LAMB trust-ratio update (AdamW.trust_ratio) against the plain fused AdamW update on the full model's arena.

The full model of the bench's default workload (about 250 M parameters, every tensor given a random gradient so that all of them are in
the arena; no forward or backward pass is run), one optimizer, and two ways of launching its update over every launch class on the same
arenas in the same process: the plain update (one launch per class, 28 bytes per parameter) and the LAMB update (ytvln_lamb_stage1 ->
ytvln_lamb_trust -> ytvln_lamb_stage2 per class, 40 bytes per parameter).  Protocol of DESIGN.md section 5, shared with
tools/grad_clip_cost.py: every pass starts behind 0.4 s of GEMM (warm clocks), the configurations are interleaved, the order is reversed
every pass, min of the passes; a reading is the mean of `--reps` updates between two HIP events.  The three LAMB launches are also timed
alone.  Writes profiles/lamb_cost.json (or --out).

    python tools/lamb_cost.py [--reps 20] [--passes 3] [--out profiles/lamb_cost.json]"""
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


def build(dev):
    import bench
    from ytvln.lily import Lily
    from ytvln.vilbert import BertConfig
    from ytvln.vilbert_init import get_optimization
    cfgname, _, _, _, _, _, flags = bench.WORKLOADS["cfg2_full_pretrain_bs8"]
    args = bench.make_args(flags)
    cfg = BertConfig.from_json_file(os.path.join(ROOT, "youtube-vln_amd", "configs", cfgname))
    cfg.args = args
    torch.manual_seed(1234)
    model = Lily(cfg).to(dev).train()
    opt, _, _, _ = get_optimization(args, model, 10000, None)
    for g in opt.param_groups:
        g["lr"] = 1e-5          # (a schedule's warm-up would start at 0)
    gen = torch.Generator(device=dev).manual_seed(5)
    for p in model.parameters():
        p.grad = torch.empty_like(p).normal_(generator=gen).mul_(1e-3)
    opt.step()                  # builds the arenas and the launch classes, uploads the hyper-parameters
    torch.cuda.synchronize()
    return model, opt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lamb_cost.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    from ytvln import ops
    model, opt = build(dev)
    arena = opt._arena
    elems = sum(numel for _, numel in arena["index"].values())
    opt.lamb_buffers()

    def plain():
        opt.trust_ratio = False
        opt.launch_classes()

    def lamb():
        opt.trust_ratio = True
        opt.launch_classes()
    t = protocol(dev, {"adamw": plain, "lamb": lamb}, a.reps, a.passes)
    partials, trust, report = opt.lamb_buffers()
    g = opt.flat_grad()

    def parts(c):
        return partials[2 * c["rec0"]:2 * (c["rec0"] + c["n"])]

    def stage1():
        for c in opt._launch:
            ops.lamb_stage1(arena["p"], g, arena["m"], arena["v"], c["table"], c["n"], c["hyper"], parts(c), opt.grad_scale, None)

    def trust_only():
        for c in opt._launch:
            ops.lamb_trust(parts(c), c["table"], c["n"], c["tensor_first"], c["rec_tensor"], c["ntensors"], trust, report, None)

    def stage2():
        for c in opt._launch:
            ops.lamb_stage2(arena["p"], arena["m"], arena["v"], c["table"], c["n"], c["hyper"], trust, c["rec_tensor"], None, p_bf16=arena["pb"])
    alone = protocol(dev, {"lamb_stage1": stage1, "lamb_trust": trust_only, "lamb_stage2": stage2}, a.reps, a.passes)
    torch.cuda.synchronize()
    res = {"model": "cfg2_full_pretrain_bs8", "parameters": elems, "arena_elements": int(arena["p"].numel()), "tensors": len(arena["index"]),
           "launch_classes": len(opt._launch), "records": sum(c["n"] for c in opt._launch), "reps_per_reading": a.reps, "passes": a.passes,
           "protocol": "0.4 s of GEMM before every pass, interleaved, order reversed every pass, min of the passes", "update_ms": {}}
    for name, nbytes in (("adamw", 28), ("lamb", 40)):
        v = t[name]
        res["update_ms"][name] = {"min": min(v), "passes": v, "spread": max(v) - min(v), "bytes_per_parameter": nbytes,
                                  "tb_per_s": nbytes * elems / (min(v) * 1e-3) / 1e12}
    res["ratio_lamb_over_adamw"] = res["update_ms"]["lamb"]["min"] / res["update_ms"]["adamw"]["min"]
    res["ratio_by_bytes"] = 40 / 28
    for name, nbytes in (("lamb_stage1", 24), ("lamb_trust", 0), ("lamb_stage2", 16)):
        v = alone[name]
        res[name] = {"ms": min(v), "passes": v}
        if nbytes:
            res[name].update(bytes_per_parameter=nbytes, tb_per_s=nbytes * elems / (min(v) * 1e-3) / 1e12,
                             fraction_of_8_tb_per_s=nbytes * elems / (min(v) * 1e-3) / 1e12 / PEAK_HBM_TBS)
    res["parameters_finite"] = bool(torch.isfinite(arena["p"]).all())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
