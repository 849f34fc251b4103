#!/usr/bin/env python3
"""Cost of the stats forms of the CE / KL loss kernels (csrc/loss.hip: label smoothing, row arg-max, hits and counts from the pass that
computes the log-sum-exp) at the sizes of the benchmark configurations:

  lm_f32    [4480, 30522]  fp32 logits   (cfg 2: 56 pairs x 80 tokens)     language cross entropy
  lm_bf16   [17920, 30522] bf16 logits   (cfg 5)                           the same on the bf16-resident path
  vision    [16072, 1601]  fp32 logits   (cfg 2: 56 pairs x 287 regions)   masked KL

`--live` of the rows (default 0.15, the masking rate) carry a target; the others take the kernels' block-uniform early exit.  Per shape,
every timing a replayed graph (device time only):
  (a) plain_fwd / plain_bwd              ytvln_ce_fwd_* / ytvln_ce_bwd_* (ytvln_kl_*): what the step launches with both settings off
  (b) stats_fwd / smooth_bwd             ytvln_ce_stats_fwd_* with label_smoothing 0.1 / ytvln_ce_smooth_bwd_* (ytvln_kl_stats_fwd_*; the KL has
                                         no backward of its own)
  (c) plain_fwd_argmax                   (a)'s forward followed by torch.argmax over the same logits: the second pass the stats form replaces
Protocol of DESIGN.md section 5 (shared with tools/grad_clip_cost.py): every pass starts behind 0.4 s of GEMM, the configurations are
interleaved, the order is reversed every pass, min of the passes; a reading is the mean of `--reps` replays between two HIP events.  Beside
each time: the bytes the algorithm has to move and the fraction of 8 TB/s they amount to.  Writes profiles/loss_stats_cost.json (or --out).

    python tools/loss_stats_cost.py [--reps 20] [--passes 3] [--live 0.15] [--out profiles/loss_stats_cost.json]"""
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
from heads_cost import graphed  # noqa: E402

EPS = 0.1


def ce_case(dev, M, V, dtype, live):
    from ytvln import ops
    kind = "bf16" if dtype == torch.bfloat16 else "f32"
    ld = -(-V // 8) * 8
    buf = torch.empty(M, ld, device=dev, dtype=dtype)
    for r in range(0, M, 1024):          # filled in slabs: no fp32 temporary of the whole bf16 matrix
        buf[r:r + 1024] = torch.randn(min(1024, M - r), ld, device=dev).to(dtype)
    logits = buf[:, :V]
    g = torch.Generator(device=dev).manual_seed(1)
    target = torch.randint(0, V, (M,), device=dev, generator=g)
    target[torch.rand(M, device=dev, generator=g) >= live] = -1
    n_live = int((target != -1).sum())
    f = lambda *s: torch.empty(*s, device=dev)          # noqa: E731
    row_lse, row_nv, row_loss, out2, out4, gout = f(M), f(M), f(M), f(2), f(4), torch.ones(1, device=dev)
    row_top = torch.empty(M, dtype=torch.int64, device=dev)
    dl = torch.empty(M, ld, device=dev, dtype=dtype)
    st = ops._stream
    P = lambda t: t.data_ptr()          # noqa: E731

    def plain_fwd():
        ops.call("ytvln_ce_fwd_" + kind, P(buf), ld, P(target), -1, P(row_lse), P(row_loss), P(out2), M, V, st())

    def stats_fwd():
        ops.call("ytvln_ce_stats_fwd_" + kind, P(buf), ld, P(target), -1, EPS, P(row_lse), P(row_nv), P(row_loss), P(row_top), P(out4), M, V, st())

    def plain_fwd_argmax():
        plain_fwd()
        return torch.argmax(logits, 1)

    def plain_bwd():
        ops.call("ytvln_ce_bwd_" + kind, P(buf), ld, P(target), -1, P(row_lse), P(out2), P(gout), P(dl), ld, M, V, st())

    def smooth_bwd():
        ops.call("ytvln_ce_smooth_bwd_" + kind, P(buf), ld, P(target), -1, EPS, P(row_lse), P(row_nv), P(out4), P(gout), P(dl), ld, M, V, st())

    es = buf.element_size()
    row = n_live * V * es
    byts = {"plain_fwd": row + 16 * M, "stats_fwd": row + 28 * M, "plain_fwd_argmax": row + 16 * M + M * V * es + 8 * M,
            "plain_bwd": row + 12 * M + M * (ld if es == 2 else V) * es, "smooth_bwd": row + 16 * M + M * (ld if es == 2 else V) * es}
    fns = {"plain_fwd": plain_fwd, "stats_fwd": stats_fwd, "plain_fwd_argmax": plain_fwd_argmax, "plain_bwd": plain_bwd, "smooth_bwd": smooth_bwd}
    stats_fwd()          # the smoothing backward reads the stats forward's outputs
    plain_fwd()
    return fns, byts, n_live, (buf, target, row_lse, row_nv, row_loss, out2, out4, gout, row_top, dl)


def kl_case(dev, M, C, live):
    from ytvln import ops
    pred = torch.randn(M, C, device=dev)
    tgt = torch.softmax(torch.randn(M, C, device=dev) * 3, -1)
    g = torch.Generator(device=dev).manual_seed(2)
    mask = (torch.rand(M, device=dev, generator=g) < live).long()
    n_live = int(mask.sum())
    f = lambda *s: torch.empty(*s, device=dev)          # noqa: E731
    row_lse, row_loss, row_hit, out2, out4, gout = f(M), f(M), f(M), f(2), f(4), torch.ones(1, device=dev)
    row_top = torch.empty(M, dtype=torch.int64, device=dev)
    dp = torch.empty(M, C, device=dev)
    st = ops._stream
    P = lambda t: t.data_ptr()          # noqa: E731

    def plain_fwd():
        ops.call("ytvln_kl_fwd_f32", P(pred), C, P(tgt), C, P(mask), P(row_lse), P(row_loss), P(out2), M, C, st())

    def stats_fwd():
        ops.call("ytvln_kl_stats_fwd_f32", P(pred), C, P(tgt), C, P(mask), P(row_lse), P(row_loss), P(row_top), P(row_hit), P(out4), M, C, st())

    def plain_fwd_argmax():
        plain_fwd()
        return torch.argmax(pred, 1)

    def plain_bwd():
        ops.call("ytvln_kl_bwd_f32", P(pred), C, P(tgt), C, P(mask), P(row_lse), P(out2), P(gout), P(dp), C, M, C, st())

    row = n_live * C * 8
    byts = {"plain_fwd": row + 16 * M, "stats_fwd": row + 28 * M, "plain_fwd_argmax": row + 16 * M + M * C * 4 + 8 * M,
            "plain_bwd": row + 12 * M + M * C * 4}
    fns = {"plain_fwd": plain_fwd, "stats_fwd": stats_fwd, "plain_fwd_argmax": plain_fwd_argmax, "plain_bwd": plain_bwd}
    return fns, byts, n_live, (pred, tgt, mask, row_lse, row_loss, row_hit, out2, out4, gout, row_top, dp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--live", type=float, default=0.15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_stats_cost.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cases = {"lm_f32": ce_case(dev, 4480, 30522, torch.float32, a.live), "lm_bf16": ce_case(dev, 17920, 30522, torch.bfloat16, a.live),
             "vision": kl_case(dev, 16072, 1601, a.live)}
    configs, bytes_of = {}, {}
    for shape, (fns, byts, _, _) in cases.items():
        for n, fn in fns.items():
            configs[f"{shape}/{n}"] = graphed(fn)
            bytes_of[f"{shape}/{n}"] = byts[n]
    t = protocol(dev, configs, a.reps, a.passes)
    torch.cuda.synchronize()
    res = {"shapes": {"lm_f32": [4480, 30522], "lm_bf16": [17920, 30522], "vision": [16072, 1601]}, "label_smoothing": EPS,
           "rows_with_a_target": {s: c[2] for s, c in cases.items()}, "live_fraction": a.live, "reps_per_reading": a.reps, "passes": a.passes,
           "protocol": "replayed graphs; 0.4 s of GEMM before every pass, interleaved, order reversed every pass, min of the passes", "ms": {},
           "ratios": {}}
    for name, v in t.items():
        alg = bytes_of[name]
        res["ms"][name] = {"min": min(v), "passes": v, "spread": max(v) - min(v), "algorithmic_bytes": alg,
                           "algorithmic_tb_per_s": alg / (min(v) * 1e-3) / 1e12, "fraction_of_8_tb_per_s": alg / (min(v) * 1e-3) / 1e12 / PEAK_HBM_TBS}
    ms = lambda s, n: res["ms"][f"{s}/{n}"]["min"]          # noqa: E731
    for s in cases:
        r = {"stats_fwd_over_plain_fwd": ms(s, "stats_fwd") / ms(s, "plain_fwd"),
             "stats_fwd_over_plain_fwd_argmax": ms(s, "stats_fwd") / ms(s, "plain_fwd_argmax")}
        if f"{s}/smooth_bwd" in res["ms"]:
            r["smooth_bwd_over_plain_bwd"] = ms(s, "smooth_bwd") / ms(s, "plain_bwd")
        res["ratios"][s] = r
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
