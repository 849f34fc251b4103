#!/usr/bin/env python3
"""Step time and peak memory of activation recomputation (BertEncoder.recompute = "none" | "ffn" | "layer").

Two workloads of bench.py, each as ONE model and optimizer whose encoder attribute is switched between the tiers (the tiers are
bit-identical, so the model's trajectory does not depend on the order): the headline workload (cfg2_full_pretrain_bs8, fp32) under
"none", "ffn" and "layer", and BASELINE configs[4] at its own size (cfg5_long_traj_bs32, bf16-resident) under "none" and "layer" (the FFN
tier is fp32 only).  Eager utils_init.train_step, dropout on -- a recomputing backward is not captured into hipGraphs, so the graph-replayed
step of the bench is not what is compared here.  Protocol of DESIGN.md section 5: every pass starts behind 0.4 s of GEMM (warm clocks), the
tiers are interleaved, the order is reversed every pass; a reading is the mean of `--reps` steps between two HIP events, the figure of a
tier is the MEDIAN of its readings and the run-to-run spread the max - min of them.  Peak memory is torch.cuda.max_memory_allocated() over a
reading, the statistics reset right before it.

On a tree without the feature only "none" is measured: run there with --out elsewhere and hand that file to --parent here; the parent's
"none" is then recorded beside this tree's, with whether the two medians agree within the larger of the two spreads.  Reads nothing
outside the tree.  Writes profiles/recompute_cost.json (or --out).

    python tools/recompute_cost.py [--reps 3] [--passes 3] [--workloads cfg2,cfg5] [--parent FILE] [--out profiles/recompute_cost.json]"""
import argparse
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "youtube-vln_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from grad_clip_cost import timed, warm  # noqa: E402

WORKLOADS = {"cfg2": ("cfg2_full_pretrain_bs8", "fp32", ("none", "ffn", "layer")),
             "cfg5": ("cfg5_long_traj_bs32", "bf16", ("none", "layer"))}


def measure(dev, name, precision, tiers, reps, passes):
    import bench
    from ytvln import ops, synth, utils_init
    from ytvln.lily import Lily
    from ytvln.vilbert import BertConfig, BertEncoder
    from ytvln.vilbert_init import get_optimization
    has = hasattr(BertEncoder, "recompute")
    if not has:
        tiers = ("none",)
    cfgname, bs, K, T, frames, boxes, flags = bench.WORKLOADS[name]
    args = bench.make_args(flags)
    cfg = BertConfig.from_json_file(os.path.join(ROOT, "youtube-vln_amd", "configs", cfgname))
    cfg.args = args
    ops.set_matmul_precision(precision)
    torch.manual_seed(1234)
    model = Lily(cfg).to(dev).train()
    batch = synth.to_torch(synth.make_batch(bs=bs, K=K, T=T, frames=frames, boxes=boxes, seed=1234), dev)
    opt, sched, _, _ = get_optimization(args, model, 10000, None)
    count = [0]

    def step():
        utils_init.train_step(model, opt, sched, batch, args, count[0], all_options=True)
        count[0] += 1

    def use(tier):
        if has:
            model.bert.encoder.recompute = tier

    for tier in tiers:          # untimed: arenas, allocator, every shape of every tier
        use(tier)
        step()
        step()
    torch.cuda.synchronize()
    ms, peak = {t: [] for t in tiers}, {t: [] for t in tiers}
    for k in range(passes):
        warm(dev)
        for tier in (tiers if k % 2 == 0 else tuple(reversed(tiers))):
            use(tier)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            ms[tier].append(timed(step, reps))
            peak[tier].append(torch.cuda.max_memory_allocated(dev))
            print(f"[recompute_cost] {name} {precision} pass {k} {tier}: {ms[tier][-1]:.2f} ms/step, peak {peak[tier][-1] / 2**30:.2f} GiB",
                  file=sys.stderr, flush=True)
    use("none")
    res = {"workload": name, "precision": precision, "pairs": bs * K, "tokens": T, "regions": frames * boxes, "feature_present": has,
           "live_bytes_outside_a_step": torch.cuda.memory_allocated(dev), "tiers": {}}
    for tier in tiers:
        med = statistics.median(ms[tier])
        res["tiers"][tier] = {"step_ms_median": med, "step_ms_readings": ms[tier], "step_ms_spread": max(ms[tier]) - min(ms[tier]),
                              "pairs_per_s": 1e3 * bs * K / med, "peak_bytes": max(peak[tier]), "peak_bytes_readings": peak[tier]}
    base = res["tiers"]["none"]
    for tier in tiers[1:]:
        r = res["tiers"][tier]
        r["step_ratio_to_none"] = r["step_ms_median"] / base["step_ms_median"]
        r["peak_bytes_saved"] = base["peak_bytes"] - r["peak_bytes"]
        r["peak_ratio_to_none"] = r["peak_bytes"] / base["peak_bytes"]
    del model, opt, sched, batch
    gc.collect()
    torch.cuda.empty_cache()
    ops.set_matmul_precision("fp32")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--workloads", default="cfg2,cfg5")
    ap.add_argument("--parent", default=None, help="the file this tool wrote on the parent commit (its 'none' numbers are recorded beside this tree's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recompute_cost.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("recompute_cost: needs a HIP device (a CPU run says nothing about step time or device memory)")
    dev = torch.device("cuda", 0)
    res = {"tool": "tools/recompute_cost.py", "step": "eager utils_init.train_step, dropout on, two-stream on",
           "protocol": "0.4 s of GEMM before every pass, tiers interleaved, order reversed every pass, median of the passes; "
                       "peak = max_memory_allocated over a reading", "reps_per_reading": a.reps, "passes": a.passes, "workloads": {}}
    for key in [k for k in a.workloads.split(",") if k]:
        name, precision, tiers = WORKLOADS[key]
        res["workloads"][name] = measure(dev, name, precision, tiers, a.reps, a.passes)
    if a.parent:
        parent = json.load(open(a.parent))
        for name, w in res["workloads"].items():
            pw = parent.get("workloads", {}).get(name)
            if pw is None:
                continue
            mine, theirs = w["tiers"]["none"], pw["tiers"]["none"]
            spread = max(mine["step_ms_spread"], theirs["step_ms_spread"])
            delta = mine["step_ms_median"] - theirs["step_ms_median"]
            w["parent_none"] = {"feature_present": pw["feature_present"], "step_ms_median": theirs["step_ms_median"],
                                "step_ms_readings": theirs["step_ms_readings"], "step_ms_spread": theirs["step_ms_spread"],
                                "peak_bytes": theirs["peak_bytes"], "delta_ms_this_minus_parent": delta, "spread_ms_larger_of_the_two": spread,
                                "none_matches_parent_within_spread": abs(delta) <= spread,
                                "peak_bytes_equal": mine["peak_bytes"] == theirs["peak_bytes"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
