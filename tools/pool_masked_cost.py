#!/usr/bin/env python3
"""Cost of the frame pools' fused expansions (ytvln.batch expand_ragged_masked / expand_records_masked: region masking, and the bf16
rounding of the features, in the expansion's launch) against the unchanged composition on the same tree -- expand + randomize_regions,
and for bf16 also the ytvln_cast_f32_bf16 the bf16-resident model runs on the features -- at the shapes of tools/record_pool_cost.py,
F = 2048, C = 1601:

  cfg1    BASELINE configs[1]: bs 8, K 7, 8 frames x 36 boxes    (56 pairs x 288 regions)    masked vision, fp32 and bf16 features
  cfg4    BASELINE configs[4]: bs 32, K 7, 16 frames x 36 boxes  (224 pairs x 576 regions)   masked vision, fp32 and bf16 features
  rerank  beam re-ranking: 1 instruction x 30 beams x 8 viewpoints x 101 regions             masking off, no probabilities, bf16 features

Both pools, filled as tools/record_pool_cost.py fills them.  Every variant is captured into a HIP graph of its own (all of them are
capturable) and a reading is the mean device time of `--reps` replays between two HIP events, so the host's launch overhead is not part
of it; otherwise the protocol of DESIGN.md section 5 (0.4 s of GEMM before every pass, the variants alternate, the order is reversed every
pass, min of the passes, spread = max - min of a variant's passes).  Per variant also: the bytes it moves, derived from the shapes and from
the selected / zeroed row counts of one run, and the share of the achievable HBM rate that makes; per shape the size of the static step
inputs in each form, and whether the fused outputs equal the composition's bit for bit under the same seed.
Writes profiles/pool_masked_cost.json (or --out).  GPU only.

    python tools/pool_masked_cost.py [--reps 100] [--passes 3] [--shapes cfg1,cfg4,rerank] [--out profiles/pool_masked_cost.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "youtube-vln_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from grad_clip_cost import protocol  # noqa: E402
from ragged_pool_cost import ACHIEVABLE_HBM_TBS  # noqa: E402
from record_pool_cost import SHAPES, C, F, T, build_store, fill_ragged, fill_record  # noqa: E402

BF16 = torch.bfloat16


def capture(fn):
    """`fn` captured into a graph after one warm-up call on a side stream; returns the replay function (the graph stays alive with it)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = fn()

    def replay():
        graph.replay()
    replay.keep = (graph, keep)
    return replay


def nbytes(tensors):
    return sum(t.numel() * t.element_size() for t in tensors if t is not None)


def one_pool(kind, pool, index, view, boxes, masked, dev, reps, passes):
    from ytvln import batch as B
    from ytvln import ops
    bs, K, frames = index.shape
    R, N = frames * boxes, index.numel() * boxes
    probs = pool.probs if masked else None
    side = pool.locations if kind == "ragged" else pool.geom
    side_cols = side.shape[1]

    def f32(w):
        return torch.empty(bs, K, R, w, device=dev)

    def i64():
        return torch.empty(bs, K, R, dtype=torch.int64, device=dev)
    unfused = [f32(F), f32(12), f32(C) if masked else None, i64()]
    fused = {torch.float32: [f32(F), f32(12), f32(C) if masked else None, i64(), i64() if masked else None],
             BF16: [torch.empty(bs, K, R, F, dtype=BF16, device=dev), f32(12), f32(C) if masked else None, i64(), i64() if masked else None]}

    def expand():
        if kind == "ragged":
            return B.expand_ragged(pool.features, pool.locations, probs, pool.offsets, index, boxes, out=unfused, bad=pool.bad)
        B.global_rows(pool.features, pool.offsets, out=pool.global_features)
        return B.expand_records(pool.features, pool.geom, probs, pool.global_features, pool.offsets, index, boxes, view=view, out=unfused, bad=pool.bad)

    def composition(bf16):
        f, bx, pr, m = expand()
        tg = tm = None
        if masked:
            f, tg, tm = B.randomize_regions(f, pr, m)
        return (ops.cast_bf16(f) if bf16 else f), bx, tg, m, tm

    def fusion(dtype):
        if kind == "ragged":
            return B.expand_ragged_masked(pool.features, pool.locations, probs, pool.offsets, index, boxes, masked_vision=masked,
                                          feature_dtype=dtype, out=fused[dtype], bad=pool.bad)
        B.global_rows(pool.features, pool.offsets, out=pool.global_features)
        return B.expand_records_masked(pool.features, pool.geom, probs, pool.global_features, pool.offsets, index, boxes, view=view,
                                       masked_vision=masked, feature_dtype=dtype, out=fused[dtype], bad=pool.bad)

    # same seed, same outputs; the counts of one draw for the byte model
    agree = {}
    for name, dtype in (("fp32", torch.float32), ("bf16", BF16)):
        ops.DropoutState.manual_seed(1234)
        want = [None if t is None else t.clone() for t in composition(dtype == BF16)]
        ops.DropoutState.manual_seed(1234)
        got = fusion(dtype)
        agree[name] = all((g is None and w is None) or torch.equal(g, w) for g, w in zip(got, want))
    real = int(got[3].sum())
    sel = int(got[4].sum()) if masked else 0
    zeroed = int(((got[0] == 0).all(-1) & (got[3] == 1)).sum()) if masked else 0
    del want
    ops.DropoutState.manual_seed(None)

    variants = {}
    if masked:
        variants["unfused_fp32"] = lambda: composition(False)
        variants["fused_fp32"] = lambda: fusion(torch.float32)
    variants["unfused_bf16"] = lambda: composition(True)
    variants["fused_bf16"] = lambda: fusion(BF16)
    t = protocol(dev, {n: capture(fn) for n, fn in variants.items()}, reps, passes)
    torch.cuda.synchronize()

    # bytes: the pool rows read, the padded tensors written (and re-read by the later passes of the composition); global_rows (records) reads
    # the pool's features once more and is part of both sides
    glob = pool.rows * F * 4 + pool.frames * F * 4 if kind == "records" else 0
    small = N * (12 * 4 + 8)                                             # boxes + masks, written once by every variant
    expand_b = glob + real * (F + side_cols + (C if masked else 0)) * 4 + N * (F + (C if masked else 0)) * 4 + small
    regions_b = (N * 8 + sel * C * 4 + N * C * 4 + N * 8 + zeroed * F * 4) if masked else 0
    cast_b = N * F * 4 + N * F * 2
    fused_b = glob + (real - zeroed) * F * 4 + real * side_cols * 4 + sel * C * 4 + small + ((N * C * 4 + N * 8) if masked else 0)
    moved = {"unfused_fp32": expand_b + regions_b, "unfused_bf16": expand_b + regions_b + cast_b, "fused_fp32": fused_b + N * F * 4,
             "fused_bf16": fused_b + N * F * 2}
    entry = {"pool_rows": pool.rows, "pool_frames": pool.frames, "padded_rows": N, "real_rows": real, "selected_rows": sel, "zeroed_rows": zeroed,
             "bad_slots": int(pool.bad), "fused_equals_composition_bit_for_bit": agree, "device_us": {}}
    for n, v in t.items():
        us = 1e3 * min(v)
        entry["device_us"][n] = {"us": us, "passes_us": [1e3 * x for x in v], "spread_us": 1e3 * (max(v) - min(v)), "bytes_moved": moved[n],
                                 "tb_per_s": moved[n] / us / 1e6, "share_of_achievable_hbm": moved[n] / us / 1e6 / ACHIEVABLE_HBM_TBS}
    d = entry["device_us"]
    for name in ("fp32", "bf16"):
        if "fused_" + name in d and "unfused_" + name in d:
            entry[f"fused_minus_unfused_{name}_us"] = d["fused_" + name]["us"] - d["unfused_" + name]["us"]
            entry[f"fused_over_unfused_{name}"] = d["fused_" + name]["us"] / d["unfused_" + name]["us"]
    entry["static_step_input_bytes"] = {"unfused": nbytes(unfused), "fused_fp32": nbytes(fused[torch.float32]), "fused_bf16": nbytes(fused[BF16])}
    return entry


def one_shape(name, dev, reps, passes):
    from ytvln import batch as B
    from ytvln import features as FR
    from ytvln import synth
    bs, K, frames, boxes, viewpoints = SHAPES[name]
    pano = viewpoints > 0
    frames_list, options, _, _, view = synth.make_record_pool(bs, K, T, frames, boxes, F=F, C=C, seed=4321, viewpoints=viewpoints)
    store, keys = build_store(frames_list, pano)
    reader = (FR.PanoFeaturesReader if pano else FR.BnBFeaturesReader)(store)
    P = len(frames_list)
    slots = None
    if pano:                               # every shown slot: (viewpoint, heading, next heading)
        slots = [(v, float(view[i, k, pos, 0]), float(view[i, k, pos, 1])) for i, item in enumerate(options) for k, o in enumerate(item)
                 for pos, v in enumerate(o[:frames])]
    ragged = B.RaggedPool((len(slots) if pano else P) * boxes, len(slots) if pano else P, feature_dim=F, num_classes=C, device=dev)
    record = B.RecordPool(sum(len(fr[0]) for fr in frames_list), P, feature_dim=F, num_classes=C, device=dev)
    rid, vid = fill_ragged(ragged, reader, keys, slots, boxes), fill_record(record, reader, keys, slots)
    if pano:                               # the ids come back slot by slot, in the order the options were walked
        it_r, it_v = iter(rid), iter(vid)
        ragged_options = [[[next(it_r) for _ in o[:frames]] for o in item] for item in options]
        record_options = [[[next(it_v) for _ in o[:frames]] for o in item] for item in options]
    else:
        ragged_options = record_options = options
    index_r, index_v = B.RaggedPool.index(ragged_options, frames).to(dev), B.RecordPool.index(record_options, frames).to(dev)
    view_dev = torch.from_numpy(view).to(dev) if pano else None
    ragged.upload()
    record.upload()
    masked = not pano                      # the masked-vision variants belong to the training shapes; re-ranking: masking off, no probabilities
    return {"bs": bs, "K": K, "frames": frames, "boxes": boxes, "F": F, "C": C, "slots": bs * K * frames, "masked_vision": masked,
            "ragged": one_pool("ragged", ragged, index_r, None, boxes, masked, dev, reps, passes),
            "records": one_pool("records", record, index_v, view_dev, boxes, masked, dev, reps, passes)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--shapes", default="cfg1,cfg4,rerank")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_masked_cost.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU only"
    dev = torch.device("cuda", 0)
    res = {"command": " ".join(["python", "tools/pool_masked_cost.py"] + sys.argv[1:]), "reps_per_reading": a.reps, "passes": a.passes,
           "achievable_hbm_tb_per_s": ACHIEVABLE_HBM_TBS, "unit": "microseconds of device time per call (graph replay)",
           "protocol": "every variant captured into a HIP graph of its own; 0.4 s of GEMM before every pass, the variants alternate, order reversed "
                       "every pass, a reading = the mean of the replays between two HIP events, min of the passes; spread = max - min",
           "variants": {"unfused_fp32": "pool expand (records: global_rows first) + randomize_regions: the composition mask_batch runs today",
                        "unfused_bf16": "the same + ytvln_cast_f32_bf16 of the features, which the bf16-resident model runs on its fp32 input "
                                        "(re-ranking shape: expand without probabilities + the cast)",
                        "fused_fp32": "expand_*_masked(feature_dtype=torch.float32): one launch (records: global_rows first)",
                        "fused_bf16": "expand_*_masked(feature_dtype=torch.bfloat16) (re-ranking shape: masked_vision=False, no probabilities)"},
           "bytes_moved": "derived from the shapes and from the real / selected / zeroed row counts of one run, not measured", "shapes": {}}
    for name in a.shapes.split(","):
        res["shapes"][name] = one_shape(name, dev, a.reps, a.passes)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
