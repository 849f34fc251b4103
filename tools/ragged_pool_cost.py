#!/usr/bin/env python3
"""Cost of building the padded batch from a ragged frame pool in one launch (ytvln.batch.expand_ragged(out=static)) against today's path:
expand_options on the same content padded to `boxes` rows per frame, plus the copy_ of its four results into the static tensors a
graph-replayed step reads (bench.py's compact variant).

Two shapes, F = 2048, C = 1601, frames of 1 .. boxes + 3 rows cut to `boxes` (synth.make_ragged_pool):
  cfg1  BASELINE configs[1]: bs 8, K 7, 8 frames x 36 boxes   (56 pairs x 288 regions)
  cfg4  BASELINE configs[4]: bs 32, K 7, 16 frames x 36 boxes (224 pairs x 576 regions)
One process; protocol of DESIGN.md section 5, shared with tools/grad_clip_cost.py: every pass starts behind 0.4 s of GEMM (warm clocks),
the two paths alternate, the order is reversed every pass; a reading is the mean of `--reps` calls between two HIP events, the spread is
max - min of a path's passes.  Recorded per shape: the times, the bytes (a) reads and writes -- computed here from the shapes and the
actual row counts -- and its bytes per second as a share of the 6.3 TB/s a float4 copy kernel reaches on an MI355X (8 TB/s peak), the
H2D bytes of the three forms a loader can ship (ragged pool, padded pool, fully padded batch), and whether the two paths computed the same
tensors.  Writes profiles/ragged_pool_cost.json (or --out).

    python tools/ragged_pool_cost.py [--reps 200] [--passes 3] [--shapes cfg1,cfg4] [--out profiles/ragged_pool_cost.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "youtube-vln_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from grad_clip_cost import protocol  # noqa: E402

SHAPES = {"cfg1": (8, 7, 8, 36), "cfg4": (32, 7, 16, 36)}          # bs, K, frames, boxes
F, C, L, T = 2048, 1601, 11, 80
ACHIEVABLE_HBM_TBS = 6.3


def bytes_of_ragged_launch(offsets, index, boxes, pool_frames):
    """(read, written) bytes of one expand_ragged launch: every output element is written once; of the pool only the first min(n, boxes)
    rows of each SHOWN frame are read, once per slot that shows them (a frame shown by several options is read again, from cache or not)."""
    idx = index.reshape(-1)
    shown = idx[(idx >= 0) & (idx < pool_frames)]
    n = np.minimum(offsets[shown + 1] - offsets[shown], boxes)
    read = int(n.sum()) * (F + L + C) * 4 + idx.size * 8 + 2 * 8 * shown.size
    written = idx.size * boxes * ((F + 12 + C) * 4 + 8)
    return read, written


def one_shape(name, dev, reps, passes):
    from ytvln import batch as B
    from ytvln import synth
    bs, K, frames, boxes = SHAPES[name]
    frames_list, options, _, _ = synth.make_ragged_pool(bs, K, T, frames, boxes, F=F, C=C, seed=4321)
    P = len(frames_list)
    pool = B.RaggedPool(P * boxes, P, feature_dim=F, loc_dim=L, num_classes=C, device=dev)
    for i, fr in enumerate(frames_list):
        pool.add(i, *fr, max_rows=boxes)
    host_index = B.RaggedPool.index(options, frames)
    index = host_index.to(dev)
    pool.upload()
    R = frames * boxes
    static = [torch.empty(bs, K, R, w, device=dev) for w in (F, 12, C)] + [torch.empty(bs, K, R, dtype=torch.int64, device=dev)]
    targets = [[torch.empty_like(t) for t in static]]          # path (b) writes a second set first, so that the two results can be compared

    # the same content padded on the host, as make_pool ships it
    offs = pool.host_offsets.numpy()[:P + 1].copy()
    pf, pb, pp = np.zeros((P, boxes, F), np.float32), np.zeros((P, boxes, 12), np.float32), np.zeros((P, boxes, C), np.float32)
    pm = np.zeros((P, boxes), np.int64)
    for p in range(P):
        a, n = offs[p], offs[p + 1] - offs[p]
        pf[p, :n], pb[p, :n, :L], pp[p, :n], pm[p, :n] = (pool.host_features[a:a + n].numpy(), pool.host_locations[a:a + n].numpy(),
                                                          pool.host_probs[a:a + n].numpy(), 1)
    padded = [torch.from_numpy(x).to(dev) for x in (pf, pb, pp, pm)]

    def ragged():
        pool.expand(index, boxes, out=static)

    def options_then_copy():
        for d, s in zip(targets[0], B.expand_options(*padded, index)):
            d.copy_(s)

    ragged()
    options_then_copy()
    torch.cuda.synchronize()
    static_b = targets[0]
    valid = (index >= 0).view(bs, K, frames, 1).expand(bs, K, frames, boxes).reshape(bs, K, R)
    same = (torch.equal(static[0], static_b[0]) and torch.equal(static[2], static_b[2]) and torch.equal(static[3], static_b[3])
            and torch.equal(static[1][..., :11], static_b[1][..., :11]) and torch.equal(static[1][..., 11][valid], static_b[1][..., 11][valid]))
    targets[0] = static                                        # timed: both paths fill the same static tensors
    del static_b
    t = protocol(dev, {"ragged": ragged, "options_then_copy": options_then_copy}, reps, passes)
    torch.cuda.synchronize()
    read, written = bytes_of_ragged_launch(offs, host_index.numpy(), boxes, P)
    entry = {"bs": bs, "K": K, "frames": frames, "boxes": boxes, "F": F, "C": C, "pool_frames": P, "pool_rows": pool.rows, "slots": bs * K * frames,
             "bad_slots": int(pool.bad), "paths_agree_outside_column_11_of_padding_frames": bool(same)}
    for n, v in t.items():
        entry[n] = {"us": 1e3 * min(v), "passes_us": [1e3 * x for x in v], "spread_us": 1e3 * (max(v) - min(v))}
    a, b = entry["ragged"], entry["options_then_copy"]
    spread = max(a["spread_us"], b["spread_us"])
    entry["ragged_minus_options_then_copy_us"] = a["us"] - b["us"]
    entry["ragged_over_options_then_copy"] = a["us"] / b["us"]
    entry["run_to_run_spread_us"] = spread
    entry["ragged_not_slower_within_spread"] = bool(a["us"] <= b["us"] + spread)
    tbs = (read + written) / (a["us"] * 1e-6) / 1e12
    entry["ragged_bytes"] = {"read": read, "written": written, "tb_per_s": tbs, "share_of_achievable_hbm": tbs / ACHIEVABLE_HBM_TBS}
    slots_rows = bs * K * R
    entry["h2d_bytes"] = {"ragged_pool": pool.bytes_uploaded + host_index.numel() * 8,
                          "padded_pool": P * boxes * ((F + 12 + C) * 4 + 8) + host_index.numel() * 8,
                          "padded_batch": slots_rows * ((F + 12 + C) * 4 + 8)}
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--shapes", default="cfg1,cfg4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_pool_cost.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU only"
    dev = torch.device("cuda", 0)
    res = {"reps_per_reading": a.reps, "passes": a.passes, "unit": "microseconds per call", "achievable_hbm_tb_per_s": ACHIEVABLE_HBM_TBS,
           "protocol": "0.4 s of GEMM before every pass, the two paths alternate, order reversed every pass, min of the passes; spread = max - min",
           "paths": {"ragged": "RaggedPool.expand(index, boxes, out=static): one launch",
                     "options_then_copy": "expand_options on the padded pool + copy_ of its four results into static tensors"},
           "shapes": {}}
    for name in a.shapes.split(","):
        res["shapes"][name] = one_shape(name, dev, a.reps, a.passes)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
