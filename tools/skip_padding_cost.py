#!/usr/bin/env python3
"""Step time of padding-free execution (BertModel.skip_padding) against the padded step, and the price of its row moves.

Two shapes of bench.py -- the headline (cfg2_full_pretrain_bs8) and BASELINE configs[4] at its own size (cfg5_long_traj_bs32) -- each in fp32
and on the bf16-resident path, each as ONE model and optimizer whose `bert.skip_padding` attribute is switched between
    padded   None (the default path)
    exact    "exact": the count of valid rows is read on the host, capacity = the count rounded up to 256
    static   the (text, image) fractions that give the same capacities without a host read, chosen from this batch's own counts
on the synth.make_batch batch of the workload (its masks follow the data: 10-36 boxes per frame, 4-8 frames, 20-78 tokens) and on the same
batch with every mask full -- the price of the feature when there is nothing to skip.  Eager utils_init.train_step, dropout on; padded and
static also as a captured hipGraph of the whole step, replayed ("exact" cannot be captured).  Protocol of DESIGN.md section 5: every pass
starts behind 0.4 s of GEMM (warm clocks), the modes are interleaved (ABAB...), the order is reversed every pass, a reading is the mean of
`--reps` steps between two HIP events, the figure of a mode is the MIN of its >= 3 readings and the spread their max - min.

The row mover alone: ytvln_rows_move_* at the widths and row counts of the image side of each shape (the q|k|v unpack and the context pack of
a self-attention site), bytes moved / time against the 8 TB/s of HBM.

Reads nothing outside the tree.  Writes profiles/skip_padding_cost.json (or --out).

    python tools/skip_padding_cost.py [--reps 2] [--passes 3] [--workloads cfg2,cfg5] [--precisions fp32,bf16] [--out FILE]"""
import argparse
import gc
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "youtube-vln_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from grad_clip_cost import protocol, timed, warm  # noqa: E402

WORKLOADS = {"cfg2": "cfg2_full_pretrain_bs8", "cfg5": "cfg5_long_traj_bs32"}
HBM_BYTES_PER_S = 8e12


def summary(readings, pairs):
    best = min(readings)
    return {"step_ms_min": best, "step_ms_readings": readings, "step_ms_spread": max(readings) - min(readings), "pairs_per_s": 1e3 * pairs / best}


def compare(res, base, other):
    a, b = res[base], res[other]
    spread = max(a["step_ms_spread"], b["step_ms_spread"])
    gain = a["step_ms_min"] - b["step_ms_min"]
    return {"ms_saved": gain, "ratio_to_" + base: b["step_ms_min"] / a["step_ms_min"], "spread_ms_larger_of_the_two": spread,
            "ahead_by_more_than_the_spread": gain > spread}


def measure(dev, name, precision, reps, passes, graphs):
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
    nb = synth.make_batch(bs=bs, K=K, T=T, frames=frames, boxes=boxes, seed=1234)
    full = [a.copy() for a in nb]
    full[7], full[3] = np.ones_like(nb[7]), np.ones_like(nb[3])
    batches = {"data": synth.to_torch(nb, dev), "full": synth.to_torch(full, dev)}
    rows_t, rows_v = int(nb[7].size), int(nb[3].size)
    count_t, count_v = int((nb[7] != 0).sum()), int((nb[3] != 0).sum())
    cap = lambda count, rows: min(rows, -(-count // 256) * 256)          # noqa: E731
    fracs = ((cap(count_t, rows_t) - 0.5) / rows_t, (cap(count_v, rows_v) - 0.5) / rows_v)          # (half a row below: no rounding into the next tile)
    assert (ops.rows_capacity(rows_t, fracs[0]), ops.rows_capacity(rows_v, fracs[1])) == (cap(count_t, rows_t), cap(count_v, rows_v))
    modes = {"padded": None, "exact": "exact", "static": fracs}
    opt, sched, _, _ = get_optimization(args, model, 10000, None)
    count = [0]

    def eager(which, mode):
        def step():
            model.bert.skip_padding = modes[mode]
            utils_init.train_step(model, opt, sched, batches[which], args, count[0], all_options=True)
            count[0] += 1
        return step

    res = {"workload": name, "precision": precision, "pairs": bs * K, "tokens": T, "regions": frames * boxes,
           "rows": {"text": rows_t, "image": rows_v}, "valid_rows": {"text": count_t, "image": count_v},
           "valid_fraction": {"text": count_t / rows_t, "image": count_v / rows_v},
           "capacity": {"text": cap(count_t, rows_t), "image": cap(count_v, rows_v)}, "static_fractions": list(fracs)}
    for which in ("data", "full"):
        names = ("padded", "exact", "static") if which == "data" else ("padded", "exact")
        configs = {m: eager(which, m) for m in names}
        for fn in configs.values():          # untimed: arenas, allocator, every shape of every mode
            fn()
        got = protocol(dev, configs, reps, passes)
        block = {m: summary(got[m], bs * K) for m in names}
        for m in names[1:]:
            block[m].update(compare(block, "padded", m))
        res["eager_" + which] = block
        print(f"[skip_padding_cost] {name} {precision} eager {which}: " + ", ".join(f"{m} {block[m]['step_ms_min']:.2f} ms" for m in names),
              file=sys.stderr, flush=True)
    assert float(model.bert.padding_overflow.sum()) == 0.0, model.bert.padding_overflow.tolist()
    if graphs:          # the whole step captured once per mode and replayed (tests/test_model_gpu.py::test_graph_replay_equals_eager's recipe)
        replay = {}
        for m in ("padded", "static"):
            model.bert.skip_padding = modes[m]
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                utils_init.train_step(model, opt, None, batches["data"], args, 0, all_options=True)

            def run(g=g):
                opt.prepare_replay()
                g.replay()
            replay[m] = run
        got = protocol(dev, replay, reps, passes)
        block = {m: summary(got[m], bs * K) for m in replay}
        block["static"].update(compare(block, "padded", "static"))
        res["graph_data"] = block
        print(f"[skip_padding_cost] {name} {precision} graph data: " + ", ".join(f"{m} {block[m]['step_ms_min']:.2f} ms" for m in block),
              file=sys.stderr, flush=True)
        del replay, g
    model.bert.skip_padding = None
    del model, opt, sched, batches
    gc.collect()
    torch.cuda.empty_cache()
    ops.set_matmul_precision("fp32")
    return res


def mover(dev, name, reps=20):
    """The row moves of one image-side self-attention site at the workload's shape: unpack of the packed q|k|v projection, pack of the context."""
    import bench
    from ytvln import ops, synth
    cfgname, bs, K, T, frames, boxes, _ = bench.WORKLOADS[name]
    hv = json.load(open(os.path.join(ROOT, "youtube-vln_amd", "configs", cfgname)))["v_hidden_size"]
    nb = synth.make_batch(bs=bs, K=K, T=T, frames=frames, boxes=boxes, seed=1234)
    mask = torch.from_numpy(nb[3]).to(dev)
    rows, count = mask.numel(), int((nb[3] != 0).sum())
    plan = ops.rows_plan(mask, min(rows, -(-count // 256) * 256))
    out = {"rows": rows, "valid_rows": count, "capacity": plan.capacity, "launches": {}}
    for dtype, es in ((torch.float32, 4), (torch.bfloat16, 2)):
        packed = torch.randn(plan.capacity, 3 * hv, device=dev).to(dtype)
        padded = torch.randn(rows, hv, device=dev).to(dtype)
        for label, fn, moved in (("unpack_qkv", lambda: ops.rows_unpack(packed, plan), (count + rows) * 3 * hv * es),
                                 ("pack_ctx", lambda: ops.rows_pack(padded, plan), (count + plan.capacity) * hv * es)):
            fn()
            warm(dev, 0.2)
            ms = min(timed(fn, reps) for _ in range(3))
            out["launches"][f"{label}_{'bf16' if es == 2 else 'f32'}"] = {
                "ms": ms, "bytes_moved": moved, "bytes_per_s": moved / (ms * 1e-3), "fraction_of_8_TB_per_s": moved / (ms * 1e-3) / HBM_BYTES_PER_S}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--workloads", default="cfg2,cfg5")
    ap.add_argument("--precisions", default="fp32,bf16")
    ap.add_argument("--no-graphs", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skip_padding_cost.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("skip_padding_cost: needs a HIP device (a CPU run says nothing about step time)")
    if a.passes < 3:
        raise SystemExit("skip_padding_cost: the protocol takes the min of at least 3 passes")
    dev = torch.device("cuda", 0)
    res = {"tool": "tools/skip_padding_cost.py", "step": "utils_init.train_step (forward, losses, backward, AdamW), dropout on, two-stream on",
           "protocol": "0.4 s of GEMM before every pass, modes interleaved, order reversed every pass, min of the passes, spread = max - min",
           "reps_per_reading": a.reps, "passes": a.passes, "steps": [], "rows_move": {}}
    for key in [k for k in a.workloads.split(",") if k]:
        res["rows_move"][WORKLOADS[key]] = mover(dev, WORKLOADS[key])
        for precision in [p for p in a.precisions.split(",") if p]:
            res["steps"].append(measure(dev, WORKLOADS[key], precision, a.reps, a.passes, not a.no_graphs))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
