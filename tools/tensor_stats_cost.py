#!/usr/bin/env python3
"""Step time with the per-tensor statistics (AdamW.tensor_stats) on against the same step with them off.

Two shapes of bench.py -- the headline (cfg2_full_pretrain_bs8) in fp32 and BASELINE configs[4] at its own size (cfg5_long_traj_bs32) on the
bf16-resident path -- each as ONE model and optimizer whose `tensor_stats` attribute is switched between False and True: eager
utils_init.train_step (dropout on), and the whole step captured into a hipGraph once per setting and replayed.  Protocol of DESIGN.md
section 5, shared with tools/grad_clip_cost.py: every pass starts behind 0.4 s of GEMM (warm clocks), the settings are interleaved, the
order is reversed every pass, a reading is the mean of `--reps` steps between two HIP events, the figure of a setting is the MIN of its
>= 3 readings and the spread their max - min.

The two statistics launches are also timed alone over every launch class of the arena (same protocol): 8 bytes per parameter with the fp32
gradient arena, 6 with the bf16 exchange buffer as the gradient operand, against the 8 TB/s of HBM.

Reads nothing outside the tree.  Writes profiles/tensor_stats_cost.json (or --out).

    python tools/tensor_stats_cost.py [--reps 2] [--passes 3] [--cases cfg2:fp32,cfg5:bf16] [--out FILE]"""
import argparse
import gc
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "youtube-vln_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from grad_clip_cost import PEAK_HBM_TBS, protocol  # noqa: E402

WORKLOADS = {"cfg2": "cfg2_full_pretrain_bs8", "cfg5": "cfg5_long_traj_bs32"}


def summary(readings, pairs):
    best = min(readings)
    return {"step_ms_min": best, "step_ms_readings": readings, "step_ms_spread": max(readings) - min(readings), "pairs_per_s": 1e3 * pairs / best}


def compare(block):
    off, on = block["off"], block["on"]
    spread = max(off["step_ms_spread"], on["step_ms_spread"])
    delta = on["step_ms_min"] - off["step_ms_min"]
    return {"delta_ms_on_minus_off": delta, "ratio_on_over_off": on["step_ms_min"] / off["step_ms_min"], "spread_ms_larger_of_the_two": spread,
            "delta_larger_than_the_spread": abs(delta) > spread}


def measure(dev, name, precision, reps, passes):
    import bench
    from ytvln import ops, synth, utils_init
    from ytvln.lily import Lily
    from ytvln.vilbert import BertConfig
    from ytvln.vilbert_init import get_optimization
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

    def eager(on):
        def step():
            opt.tensor_stats = on
            utils_init.train_step(model, opt, sched, batch, args, count[0], all_options=True)
            count[0] += 1
        return step
    configs = {"off": eager(False), "on": eager(True)}
    for fn in configs.values():          # untimed: arenas, allocator, the statistics buffers
        fn()
    elems = sum(numel for _, numel in opt._arena["index"].values())
    res = {"workload": name, "precision": precision, "pairs": bs * K, "parameters": elems, "tensors": len(opt._arena["index"]),
           "launch_classes": len(opt._launch), "records": sum(c["n"] for c in opt._launch)}
    got = protocol(dev, configs, reps, passes)
    block = {m: summary(got[m], bs * K) for m in configs}
    block.update(compare(block))
    res["eager"] = block
    print(f"[tensor_stats_cost] {name} {precision} eager: off {block['off']['step_ms_min']:.2f} ms, on {block['on']['step_ms_min']:.2f} ms",
          file=sys.stderr, flush=True)
    # the whole step captured once per setting and replayed (tests/test_model_gpu.py::test_graph_replay_equals_eager's recipe).  One
    # optimizer replays both captures, so prepare_replay()'s check of the captured setting is stepped over: its hyper-parameter upload alone.
    replay = {}
    for m, on in (("off", False), ("on", True)):
        opt.tensor_stats = on
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            utils_init.train_step(model, opt, None, batch, args, 0, all_options=True)

        def run(g=g):
            opt._upload_hyper()
            g.replay()
        replay[m] = run
    got = protocol(dev, replay, reps, passes)
    block = {m: summary(got[m], bs * K) for m in replay}
    block.update(compare(block))
    res["graph"] = block
    print(f"[tensor_stats_cost] {name} {precision} graph: off {block['off']['step_ms_min']:.2f} ms, on {block['on']['step_ms_min']:.2f} ms",
          file=sys.stderr, flush=True)
    # the two launches alone, over every launch class: with the fp32 gradient arena and with the bf16 exchange buffer as the operand
    opt.tensor_stats = True
    opt.pack_grads()

    def launches(dtype):
        def run():
            opt.exchange_dtype = dtype
            opt.tensor_stats_launch()
        return run
    alone = protocol(dev, {"g_fp32": launches(torch.float32), "g_bf16": launches(torch.bfloat16)}, 20, passes)
    opt.exchange_dtype = torch.float32
    res["launches_alone"] = {}
    for m, nbytes in (("g_fp32", 8), ("g_bf16", 6)):
        ms = min(alone[m])
        rate = nbytes * elems / (ms * 1e-3) / 1e12
        res["launches_alone"][m] = {"ms": ms, "passes": alone[m], "bytes_per_parameter": nbytes, "bytes": nbytes * elems, "tb_per_s": rate,
                                    "fraction_of_8_tb_per_s": rate / PEAK_HBM_TBS}
    torch.cuda.synchronize()
    counts = opt.tensor_stats_report()[1]
    res["nonfinite_gradient_tensors_last_step"] = int((counts[:, 0] > 0).sum())
    del replay, g, model, opt, sched, batch
    gc.collect()
    torch.cuda.empty_cache()
    ops.set_matmul_precision("fp32")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--cases", default="cfg2:fp32,cfg5:bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_stats_cost.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tensor_stats_cost: needs a HIP device (a CPU run says nothing about step time)")
    if a.passes < 3:
        raise SystemExit("tensor_stats_cost: the protocol takes the min of at least 3 passes")
    dev = torch.device("cuda", 0)
    res = {"tool": "tools/tensor_stats_cost.py", "step": "utils_init.train_step (forward, losses, backward, AdamW), dropout on",
           "protocol": "0.4 s of GEMM before every pass, settings interleaved, order reversed every pass, min of the passes, spread = max - min",
           "reps_per_reading": a.reps, "passes": a.passes, "steps": []}
    for case in [c for c in a.cases.split(",") if c]:
        key, _, precision = case.partition(":")
        res["steps"].append(measure(dev, WORKLOADS[key], precision or "fp32", a.reps, a.passes))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
