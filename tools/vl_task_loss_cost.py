#!/usr/bin/env python3
"""Cost of the VL-task loss (csrc/task_loss.hip through ops.bce_with_logits_rows): forward plus backward at

  [256, 3129]   a VQA batch: 3129 answers          [256, 101]   a grounding batch: 101 regions

with a per-class pos_weight and scale = C, and beside it, as a yardstick only, torch's own way to the same three results on the same device
tensors: F.binary_cross_entropy_with_logits (mean, times C) with its backward, plus argmax / gather / sum for the score.  Both through their
Python wrappers (host dispatch inside the window) and both as replayed graphs (device time only).  Protocol of DESIGN.md section 5 (shared
with tools/grad_clip_cost.py): every pass starts behind 0.4 s of GEMM, the configurations are interleaved, the order is reversed every pass,
min of the passes; a reading is the mean of `--reps` calls between two HIP events.  Nothing in the tests depends on these numbers.
Writes profiles/vl_task_loss_cost.json (or --out).

    python tools/vl_task_loss_cost.py [--reps 20] [--passes 3] [--out profiles/vl_task_loss_cost.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "youtube-vln_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from grad_clip_cost import protocol  # noqa: E402
from heads_cost import graphed  # noqa: E402

SHAPES = [(256, 3129), (256, 101)]


def case(dev, M, C):
    from ytvln import ops
    g = torch.Generator(device=dev).manual_seed(M + C)
    x = (3.0 * torch.randn(M, C, device=dev, generator=g)).requires_grad_(True)
    t = torch.where(torch.rand(M, C, device=dev, generator=g) < 0.02, torch.rand(M, C, device=dev, generator=g), torch.zeros((), device=dev))
    pw = 0.5 + 2.0 * torch.rand(C, device=dev, generator=g)

    def ours():
        loss, score, top = ops.bce_with_logits_rows(x, t, pw, scale=float(C))
        return (loss.detach(), score) + torch.autograd.grad(loss, [x])

    def torch_chain():
        loss = F.binary_cross_entropy_with_logits(x, t, pos_weight=pw) * C
        score = t.gather(1, torch.argmax(x.detach(), 1, keepdim=True)).sum()
        return (loss.detach(), score) + torch.autograd.grad(loss, [x])
    return ours, torch_chain, (x, t, pw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vl_task_loss_cost.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    configs, agree, keep = {}, {}, []
    for M, C in SHAPES:
        ours, chain, k = case(dev, M, C)
        keep.append(k)
        tag = f"{M}x{C}"
        lo, so, go = ours()
        lt, st_, gt = chain()
        agree[tag] = {"loss_rel": float((lo - lt).abs() / lt.abs()), "score_abs": float((so - st_).abs()),
                      "grad_rel_l2": float((go - gt).double().norm() / gt.double().norm())}
        configs.update({f"rows_{tag}": ours, f"torch_{tag}": chain, f"rows_{tag}_graph": graphed(ours), f"torch_{tag}_graph": graphed(chain)})
    t = protocol(dev, configs, a.reps, a.passes)
    torch.cuda.synchronize()
    res = {"shapes": [list(s) for s in SHAPES], "what": "forward + backward of the loss, the score included; per-class pos_weight, scale = C",
           "reps_per_reading": a.reps, "passes": a.passes,
           "protocol": "0.4 s of GEMM before every pass, interleaved, order reversed every pass, min of the passes", "ms": {},
           "agreement_rows_vs_torch": agree, "bytes_moved_rows": {}}
    for name, v in t.items():
        res["ms"][name] = {"min": min(v), "passes": v, "spread": max(v) - min(v)}
    for M, C in SHAPES:
        tag = f"{M}x{C}"
        res["bytes_moved_rows"][tag] = 2 * (2 * M * C * 4) + M * C * 4 + 2 * 16 * M          # x and t twice, dx once, the row records
        for form in ("", "_graph"):
            res[f"ratio_torch_over_rows_{tag}{form}"] = res["ms"][f"torch_{tag}{form}"]["min"] / res["ms"][f"rows_{tag}{form}"]["min"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
