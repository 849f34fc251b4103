#!/usr/bin/env python3
"""Cost of action-aware token masking (ytvln.batch.randomize_tokens(..., mask_action_rate=0.5)) against the plain randomize_tokens call.

Shapes [8, 7, 80] (the bench's default batch) and [32, 30, 80], tokens with about 8 % action words, Philox draws (production mode).  Both
calls move 40 bytes per token (24 in, 16 out: 0.18 MB and 3 MB), far too little to be bound by HBM; what differs is that the plain kernel
spreads the tokens over up to 4096 workgroups while the action form walks one item per workgroup in 256-token chunks (three phases, one
barrier per chunk).  Two readings per call and shape:
  eager  the Python call as a user makes it (wrapper + DropoutState bookkeeping + launches), mean of `--reps` calls between two HIP events;
  graph  `--graph-calls` calls captured into one hipGraph, mean per call of `--reps` replays: the device side alone.
Protocol of DESIGN.md section 5, shared with tools/grad_clip_cost.py: every pass starts behind 0.4 s of GEMM (warm clocks), the
configurations are interleaved, the order is reversed every pass, min of the passes.  The plain kernel is the yardstick.  Writes
profiles/action_masking_cost.json (or --out).

    python tools/action_masking_cost.py [--reps 200] [--passes 3] [--graph-calls 50] [--out profiles/action_masking_cost.json]"""
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

SHAPES = ((8, 7, 80), (32, 30, 80))
RATE = 0.5


def make_tokens(shape, dev, seed=1):
    from ytvln import batch as B
    rs = np.random.RandomState(seed)
    tokens = rs.randint(1000, B.VOCAB_SIZE, size=shape).astype(np.int64)
    lens = rs.randint(20, shape[-1], size=shape[:-1])
    mask = (np.arange(shape[-1]) < lens[..., None]).astype(np.int64)
    act = rs.rand(*shape) < 0.08
    tokens[act] = np.asarray(B.ACTION_TOKEN_IDS)[rs.randint(0, 3, size=int(act.sum()))]
    return torch.from_numpy(tokens * mask).to(dev), torch.from_numpy(mask).to(dev)


def captured(fn, calls):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = [fn() for _ in range(calls)]
    return graph, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--graph-calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "action_masking_cost.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU only"
    dev = torch.device("cuda", 0)
    from ytvln import batch as B
    res = {"rate": RATE, "action_share_of_tokens": 0.08, "draws": "philox", "reps_per_reading": a.reps, "passes": a.passes,
           "calls_per_graph": a.graph_calls, "unit": "microseconds per call",
           "protocol": "0.4 s of GEMM before every pass, interleaved, order reversed every pass, min of the passes", "shapes": {}}
    for shape in SHAPES:
        tok, msk = make_tokens(shape, dev)
        fns = {"plain": lambda: B.randomize_tokens(tok, msk), "action": lambda: B.randomize_tokens(tok, msk, mask_action_rate=RATE)}
        out, tgt, counts = B.randomize_tokens(tok, msk, mask_action_rate=RATE, return_counts=True)
        eager = protocol(dev, fns, a.reps, a.passes)
        graphs = {n: captured(f, a.graph_calls) for n, f in fns.items()}
        replay = protocol(dev, {n: g[0].replay for n, g in graphs.items()}, a.reps, a.passes)
        torch.cuda.synchronize()
        entry = {"tokens": tok.numel(), "bytes_moved": 40 * tok.numel(), "action_words": int(counts[:, 0].sum()), "draws": int(counts[:, 1].sum()),
                 "action_targets": int(((tgt != -1) & (out == B.MASK_TOKEN_ID)).sum())}
        for kind, t, per in (("eager", eager, 1), ("graph", replay, a.graph_calls)):
            entry[kind] = {n: {"us": 1e3 * min(v) / per, "passes_us": [1e3 * x / per for x in v], "spread_us": 1e3 * (max(v) - min(v)) / per}
                           for n, v in t.items()}
            entry[kind]["action_minus_plain_us"] = entry[kind]["action"]["us"] - entry[kind]["plain"]["us"]
            entry[kind]["action_over_plain"] = entry[kind]["action"]["us"] / entry[kind]["plain"]["us"]
        res["shapes"]["x".join(map(str, shape))] = entry
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
