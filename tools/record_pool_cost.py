#!/usr/bin/env python3
"""Cost of the raw-record frame pool (ytvln.batch.RecordPool: global_rows + expand_records on decoded records) against the ragged frame
pool (RaggedPool: expand_ragged on the readers' finished frames) at the same shapes, F = 2048, C = 1601:

  cfg1    BASELINE configs[1]: bs 8, K 7, 8 frames x 36 boxes    (56 pairs x 288 regions)    photo frames of 1 .. boxes + 3 regions
  cfg4    BASELINE configs[4]: bs 32, K 7, 16 frames x 36 boxes  (224 pairs x 576 regions)
  rerank  beam re-ranking: 1 instruction x 30 beams x 8 viewpoints x 101 regions, 40 distinct panorama viewpoints, every slot its own
          (heading, next heading); the ragged path keys its frames by (viewpoint, heading, next heading)

One process, three measurements per shape:
  device  time of RecordPool.expand (two launches) against RaggedPool.expand (one), both into the same static tensors; protocol of
          DESIGN.md section 5, shared with tools/ragged_pool_cost.py (0.4 s of GEMM before every pass, the paths alternate, the order is
          reversed every pass, a reading is the mean of `--reps` calls between two HIP events, spread = max - min of a path's passes).
          global_rows is also timed alone.  Bound: 1.10 x expand_ragged + the time to read the pool's features once at 6.3 TB/s.
  host    CPU time per step of reader[...] + RaggedPool.add against reader.records(...) + RecordPool.add over every frame of the step, on
          synthetic stores in the reference's on-disk format (time.process_time: CPU seconds of the process, all threads; the wall time next
          to it; the paths alternate, min of `--host-passes`).  Both paths unpickle and base64-decode the same records.
  h2d     bytes per step of both paths (pool + offsets + index, + view for the record path).
Also recorded: whether the two paths filled the static tensors alike (bit for bit outside the six trigonometric box columns).
Writes profiles/record_pool_cost.json (or --out).  GPU only.

    python tools/record_pool_cost.py [--reps 200] [--passes 3] [--host-passes 3] [--shapes cfg1,cfg4,rerank] [--out profiles/record_pool_cost.json]"""
import argparse
import base64
import json
import os
import pickle
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "youtube-vln_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from grad_clip_cost import protocol  # noqa: E402
from ragged_pool_cost import ACHIEVABLE_HBM_TBS  # noqa: E402

SHAPES = {"cfg1": (8, 7, 8, 36, 0), "cfg4": (32, 7, 16, 36, 0), "rerank": (1, 30, 8, 101, 40)}     # bs, K, frames, boxes, viewpoints
F, C, T = 2048, 1601, 80


def _b64(a):
    return base64.b64encode(np.ascontiguousarray(a, dtype=np.float32).tobytes())


def build_store(frames_list, pano):
    """The frames of synth.make_record_pool as a dict-backed store in the reference's on-disk format (base64 convention): one record per
    run of rows with one image size.  Returns (store, keys): keys[i] = the tuple of record keys of frame i (photo) or its one key (pano)."""
    store, keys = {}, []
    for i, (f, geom, pr) in enumerate(frames_list):
        cuts = [0] + [r for r in range(1, len(geom)) if tuple(geom[r, 4:6]) != tuple(geom[r - 1, 4:6])] + [len(geom)]
        mine = []
        for j, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            key = f"{i}-{j}"
            rec = {"image_w": int(geom[a, 4]), "image_h": int(geom[a, 5]), "features": _b64(f[a:b]), "boxes": _b64(geom[a:b, :4]),
                   "cls_prob": _b64(pr[a:b])}
            if pano:
                rec.update(vfov=60, viewHeading=_b64(np.zeros(36)), viewElevation=_b64(np.zeros(36)), featureHeading=_b64(geom[a:b, 6]),
                           featureElevation=_b64(geom[a:b, 7]), featureViewIndex=_b64(np.zeros(b - a)))
            store[key.encode()] = pickle.dumps(rec)
            mine.append(key)
        assert not pano or len(mine) == 1
        keys.append(mine[0] if pano else tuple(mine))
    store[b"keys"] = pickle.dumps(list(k for k in store))
    return store, keys


def fill_ragged(pool, reader, keys, slots, boxes):
    """One step of the ragged path.  Photo: one frame per query.  Pano (`slots` = [(viewpoint id, heading, next heading)]): one frame per
    distinct (viewpoint, heading, next heading).  Returns the pool ids in the order of `keys` / `slots`."""
    pool.reset()
    if slots is None:
        return [pool.add(q, *reader[q], max_rows=boxes) for q in keys]
    return [pool.add((v, h, nh), *reader[(keys[v], h, nh)], max_rows=boxes) for v, h, nh in slots]


def fill_record(pool, reader, keys, slots):
    pool.reset()
    if slots is None:
        return [pool.add(q, *reader.records(q)) for q in keys]
    return [pool.add(v, *reader.record(keys[v])) for v, _, _ in slots]


def host_times(fns, passes):
    """{name: [(CPU seconds of the process, all threads; wall seconds) per pass]}: the paths alternate, the order is reversed every pass."""
    out = {n: [] for n in fns}
    for k in range(passes):
        for n in (list(fns) if k % 2 == 0 else list(reversed(list(fns)))):
            c0, w0 = time.process_time(), time.perf_counter()
            fns[n]()
            out[n].append((time.process_time() - c0, time.perf_counter() - w0))
    return out


def one_shape(name, dev, reps, passes, host_passes):
    from ytvln import batch as B
    from ytvln import features as FR
    from ytvln import synth
    bs, K, frames, boxes, viewpoints = SHAPES[name]
    pano = viewpoints > 0
    frames_list, options, _, _, view = synth.make_record_pool(bs, K, T, frames, boxes, F=F, C=C, seed=4321, viewpoints=viewpoints)
    store, keys = build_store(frames_list, pano)
    reader = (FR.PanoFeaturesReader if pano else FR.BnBFeaturesReader)(store)
    P = len(frames_list)
    rows = sum(len(fr[0]) for fr in frames_list)
    slots = None
    if pano:                               # every shown slot: (viewpoint, heading, next heading)
        slots = [(v, float(view[i, k, pos, 0]), float(view[i, k, pos, 1])) for i, item in enumerate(options) for k, o in enumerate(item)
                 for pos, v in enumerate(o[:frames])]
    ragged = B.RaggedPool((len(slots) if pano else P) * boxes, len(slots) if pano else P, feature_dim=F, num_classes=C, device=dev)
    record = B.RecordPool(rows, P, feature_dim=F, num_classes=C, device=dev)

    host = host_times({"ragged": lambda: fill_ragged(ragged, reader, keys, slots, boxes), "record": lambda: fill_record(record, reader, keys, slots)},
                      host_passes)
    rid, vid = fill_ragged(ragged, reader, keys, slots, boxes), fill_record(record, reader, keys, slots)
    if pano:                               # the ids come back slot by slot, in the order the options were walked
        it_r, it_v = iter(rid), iter(vid)
        ragged_options = [[[next(it_r) for _ in o[:frames]] for o in item] for item in options]
        record_options = [[[next(it_v) for _ in o[:frames]] for o in item] for item in options]
    else:
        assert rid == vid == list(range(P))
        ragged_options = record_options = options
    ragged_index, record_index = B.RaggedPool.index(ragged_options, frames), B.RecordPool.index(record_options, frames)
    index_r, index_v = ragged_index.to(dev), record_index.to(dev)
    view_dev = torch.from_numpy(view).to(dev) if pano else None
    ragged.upload()
    record.upload()
    R = frames * boxes
    static = [torch.empty(bs, K, R, w, device=dev) for w in (F, 12, C)] + [torch.empty(bs, K, R, dtype=torch.int64, device=dev)]

    def run_ragged():
        ragged.expand(index_r, boxes, out=static)

    def run_record():
        record.expand(index_v, boxes, view=view_dev, out=static)

    def run_global_rows():
        B.global_rows(record.features, record.offsets, out=record.global_features)

    run_ragged()
    a = [t.clone() for t in static]
    run_record()
    torch.cuda.synchronize()
    trig = float((a[1][..., 5:11].double() - static[1][..., 5:11].double()).abs().max())
    same = (torch.equal(a[0], static[0]) and torch.equal(a[2], static[2]) and torch.equal(a[3], static[3])
            and torch.equal(a[1][..., :5], static[1][..., :5]) and torch.equal(a[1][..., 11], static[1][..., 11]))
    del a
    t = protocol(dev, {"ragged": run_ragged, "record": run_record, "global_rows": run_global_rows}, reps, passes)
    torch.cuda.synchronize()
    entry = {"bs": bs, "K": K, "frames": frames, "boxes": boxes, "F": F, "C": C, "slots": bs * K * frames, "distinct_frames": P,
             "ragged_pool_frames": ragged.frames, "ragged_pool_rows": ragged.rows, "record_pool_frames": record.frames, "record_pool_rows": record.rows,
             "bad_slots": int(ragged.bad) + int(record.bad), "paths_agree_bit_for_bit_outside_box_columns_5_to_10": bool(same),
             "box_columns_5_to_10_max_abs_difference": trig, "device_us": {}, "host_cpu_ms_per_step": {}}
    for n, v in t.items():
        entry["device_us"][n] = {"us": 1e3 * min(v), "passes_us": [1e3 * x for x in v], "spread_us": 1e3 * (max(v) - min(v))}
    d = entry["device_us"]
    pool_read_us = record.rows * F * 4 / (ACHIEVABLE_HBM_TBS * 1e12) * 1e6
    bound = 1.10 * d["ragged"]["us"] + pool_read_us
    entry["record_over_ragged"] = d["record"]["us"] / d["ragged"]["us"]
    entry["record_minus_ragged_us"] = d["record"]["us"] - d["ragged"]["us"]
    entry["run_to_run_spread_us"] = max(d["ragged"]["spread_us"], d["record"]["spread_us"])
    entry["pool_features_read_once_at_achievable_hbm_us"] = pool_read_us
    entry["bound_us"] = bound
    entry["record_within_bound"] = bool(d["record"]["us"] <= bound)
    for n, v in host.items():
        entry["host_cpu_ms_per_step"][n] = {"ms": 1e3 * min(c for c, _ in v), "passes_ms": [1e3 * c for c, _ in v],
                                            "wall_ms": 1e3 * min(w for _, w in v), "passes_wall_ms": [1e3 * w for _, w in v]}
    h = entry["host_cpu_ms_per_step"]
    entry["host_cpu_record_over_ragged"] = h["record"]["ms"] / h["ragged"]["ms"]
    entry["host_wall_record_over_ragged"] = h["record"]["wall_ms"] / h["ragged"]["wall_ms"]
    entry["h2d_bytes"] = {"ragged": ragged.bytes_uploaded + ragged_index.numel() * 8,
                          "record": record.bytes_uploaded + record_index.numel() * 8 + (view.size * 8 if pano else 0)}
    entry["h2d_record_over_ragged"] = entry["h2d_bytes"]["record"] / entry["h2d_bytes"]["ragged"]
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--host-passes", type=int, default=3)
    ap.add_argument("--shapes", default="cfg1,cfg4,rerank")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "record_pool_cost.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU only"
    dev = torch.device("cuda", 0)
    res = {"command": " ".join(["python", "tools/record_pool_cost.py"] + sys.argv[1:]), "reps_per_reading": a.reps, "passes": a.passes,
           "host_passes": a.host_passes, "achievable_hbm_tb_per_s": ACHIEVABLE_HBM_TBS,
           "protocol": "device: 0.4 s of GEMM before every pass, the paths alternate, order reversed every pass, min of the passes; spread = max - min.  "
                       "host: time.process_time (CPU seconds, all threads) and time.perf_counter (wall) over one step's frames, the paths "
                       "alternate, min of the passes",
           "paths": {"ragged": "reader[...] + RaggedPool.add(max_rows=boxes); RaggedPool.expand(index, boxes, out=static): one launch",
                     "record": "reader.records(...) / reader.record(key) + RecordPool.add; RecordPool.expand(index, boxes, view, out=static): "
                               "global_rows + expand_records, two launches",
                     "global_rows": "the first of the record path's two launches alone"},
           "bound": "record <= 1.10 x ragged + record_pool_rows x F x 4 bytes / achievable HBM rate", "shapes": {}}
    for name in a.shapes.split(","):
        res["shapes"][name] = one_shape(name, dev, a.reps, a.passes, a.host_passes)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
