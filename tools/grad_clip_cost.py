#!/usr/bin/env python3
"""Step-time cost of global gradient-norm clipping (AdamW.max_grad_norm / skip_nonfinite) at the headline shape.

Two replicas of the bench's default workload (full model, 56 pairs, T=80, R=288, fp32, dropout on), each with its whole training step
captured into a hipGraph: one with the feature off, one with it on (max_grad_norm=1.0, skip_nonfinite=True).  Protocol of DESIGN.md
section 5: every pass starts behind 0.4 s of GEMM (warm clocks), the configurations are interleaved, the order is reversed every pass,
min of three passes; a reading is the mean of `--replays` replays between two HIP events.  The run-to-run spread is the max - min of a
configuration's passes.  The grad_sumsq launches are also timed alone (same protocol, against 8 TB/s).  On a tree without the feature
only "off" is timed (the comparison point for "off": same tool, same box).  Writes profiles/grad_clip_cost.json (or --out).

    python tools/grad_clip_cost.py [--replays 8] [--passes 3] [--out profiles/grad_clip_cost.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "youtube-vln_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

PEAK_HBM_TBS = 8.0


def build(dev, clip):
    import bench
    from ytvln import synth, utils_init
    from ytvln.lily import Lily
    from ytvln.vilbert import BertConfig
    from ytvln.vilbert_init import get_optimization
    cfgname, bs, K, T, frames, boxes, flags = bench.WORKLOADS["cfg2_full_pretrain_bs8"]
    args = bench.make_args(flags)
    if clip:
        args.max_grad_norm, args.skip_nonfinite_grads = 1.0, True
    cfg = BertConfig.from_json_file(os.path.join(ROOT, "youtube-vln_amd", "configs", cfgname))
    cfg.args = args
    torch.manual_seed(1234)
    model = Lily(cfg).to(dev).train()
    batch = synth.to_torch(synth.make_batch(bs=bs, K=K, T=T, frames=frames, boxes=boxes, seed=1234), dev)
    opt, sched, _, _ = get_optimization(args, model, 10000, None)
    for i in range(2):
        utils_init.train_step(model, opt, sched, batch, args, i, all_options=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        utils_init.train_step(model, opt, None, batch, args, 0, all_options=True)
    torch.cuda.synchronize()

    def step():
        opt.prepare_replay()
        graph.replay()
        sched.step()
    return dict(step=step, opt=opt, keep=(model, batch, graph), pairs=bs * K)


def warm(dev, seconds=0.4):
    a = torch.randn(4096, 4096, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    while True:
        for _ in range(8):
            a @ a
        e1.record()
        e1.synchronize()
        if e0.elapsed_time(e1) >= 1e3 * seconds:
            return


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def protocol(dev, configs, reps, passes):
    """{name: [ms per pass]}: warm clocks, interleaved, order reversed every pass."""
    out = {n: [] for n in configs}
    for n in configs:
        configs[n]()          # one untimed call each
    for k in range(passes):
        warm(dev)
        for n in (list(configs) if k % 2 == 0 else list(reversed(list(configs)))):
            out[n].append(timed(configs[n], reps))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=8)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_clip_cost.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    from ytvln import ops
    from ytvln.optimization import AdamW
    has = hasattr(AdamW, "clip_settings")
    runs = {"off": build(dev, False)}
    if has:
        runs["on"] = build(dev, True)
    steps = protocol(dev, {n: r["step"] for n, r in runs.items()}, a.replays, a.passes)
    res = {"workload": "cfg2_full_pretrain_bs8", "precision": "fp32", "pairs": runs["off"]["pairs"], "replays_per_reading": a.replays,
           "passes": a.passes, "protocol": "0.4 s of GEMM before every pass, interleaved, order reversed every pass, min of the passes",
           "feature_present": has, "step_ms": {}}
    for n, v in steps.items():
        res["step_ms"][n] = {"min": min(v), "passes": v, "spread": max(v) - min(v), "pairs_per_s": 1e3 * runs[n]["pairs"] / min(v)}
    if has:
        res["delta_ms_on_minus_off"] = res["step_ms"]["on"]["min"] - res["step_ms"]["off"]["min"]
        opt = runs["on"]["opt"]
        partials, clip = opt.clip_buffers()
        g = opt.flat_grad()
        elems = sum(numel for _, numel in opt._arena["index"].values())

        def sumsq():
            opt.sumsq_tables([(ci, c["table"], c["n"]) for ci, c in enumerate(opt._launch)], 0)

        def coef():
            ops.grad_clip_coef(partials, partials.numel(), 1.0, 1.0, True, clip)
        alone = protocol(dev, {"grad_sumsq": sumsq, "grad_clip_coef": coef}, 20, a.passes)
        ms = min(alone["grad_sumsq"])
        res["grad_sumsq"] = {"ms": ms, "passes": alone["grad_sumsq"], "elements": elems, "bytes": 4 * elems, "records": int(partials.numel()),
                             "tb_per_s": 4 * elems / (ms * 1e-3) / 1e12, "fraction_of_8_tb_per_s": 4 * elems / (ms * 1e-3) / 1e12 / PEAK_HBM_TBS,
                             "arena_elements": int(g.numel())}
        res["grad_clip_coef"] = {"ms": min(alone["grad_clip_coef"]), "passes": alone["grad_clip_coef"]}
        res["skipped_steps"] = opt.skipped_steps()
        res["last_grad_norm"] = float(opt.grad_norm())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
