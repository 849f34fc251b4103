#!/usr/bin/env python3
"""Cost of the head kernels of VILBertForVLTasks (csrc/heads.hip) at the sizes of the benchmark configurations.

  row logit, fp32 rows   16128 x 1024   (cfg 2: 56 pairs x 288 regions)   forward and backward, dropout 0.1, bias and region mask
  row logit, bf16 rows   129024 x 1024  (cfg 5)                           the same
  weight norm            2048 x 1024    (SimpleClassifier's first matrix at bi_hidden 1024)   forward and backward

and, for the fp32 row logit, the three-pass way of computing the same forward values with the kernels that existed before -- ops.dropout,
ops.linear with one output column, a torch add of the mask term -- timed in the same run against the fused forward on equal terms: both
through their ops-level wrappers (host dispatch inside the window) and both as replayed graphs (device time only).  Protocol of DESIGN.md
section 5 (shared with tools/grad_clip_cost.py): every pass starts behind 0.4 s of GEMM, the configurations are interleaved, the order is reversed every pass, min of
the passes; a reading is the mean of `--reps` launches between two HIP events.  Beside each time: the bytes the algorithm has to move (every
operand once), the bytes the kernels do move (weight norm reads v twice, the row-logit backward writes and re-reads its partial rows) and the
fraction of 8 TB/s the algorithmic bytes amount to.  Writes profiles/heads_cost.json (or --out).

    python tools/heads_cost.py [--reps 20] [--passes 3] [--out profiles/heads_cost.json]"""
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


def row_logit_case(dev, rows, H, dtype, p):
    from ytvln import _lib, ops
    lib = _lib.load()
    kind = "bf16" if dtype == torch.bfloat16 else "f32"
    x = torch.randn(rows, H, device=dev).to(dtype)
    w, b = torch.randn(1, H, device=dev) * H ** -0.5, torch.zeros(1, device=dev)
    mask = (torch.rand(rows, device=dev) < 0.9).float()
    rng = torch.tensor([1234, 0], dtype=torch.int64, device=dev)
    out, dy = torch.empty(rows, device=dev), torch.randn(rows, device=dev)
    dx, dw, db = torch.empty_like(x), torch.empty(H, device=dev), torch.empty(1, device=dev)
    ws_elems = lib.ytvln_row_logit_workspace_elems(rows, H)
    ws = torch.empty(ws_elems, device=dev)
    st = ops._stream

    def fwd():
        ops.call("ytvln_row_logit_fwd_" + kind, x.data_ptr(), H, w.data_ptr(), b.data_ptr(), mask.data_ptr(), out.data_ptr(), rows, H, p,
                 rng.data_ptr(), 1, st())

    def bwd():
        ops.call("ytvln_row_logit_bwd_" + kind, x.data_ptr(), H, w.data_ptr(), dy.data_ptr(), rows, H, p, rng.data_ptr(), 1, dx.data_ptr(), H,
                 dw.data_ptr(), db.data_ptr(), ws.data_ptr(), st())

    es = x.element_size()
    byts = {"fwd": (rows * H * es + 4 * H + 8 * rows, rows * H * es + 4 * H + 8 * rows),
            "bwd": (2 * rows * H * es + 4 * rows + 8 * H, 2 * rows * H * es + 4 * rows + 8 * H + 8 * ws_elems)}
    keep = (x, w, b, mask, rng, out, dy, dx, dw, db, ws)

    # The fused forward against the three-pass form, both as a caller meets them: through the ops-level wrappers (autograd.Function.apply under
    # no_grad, output allocated per call), and both again as captured graphs, where no host dispatch is inside the timed window.
    def fused_ops():
        with torch.no_grad():
            return ops.RowLogitFn.apply(x, w, b, mask, p, rng, 1)

    def three_pass():          # the same forward values from the kernels that existed before (fp32 rows only: no dropout kernel takes bf16)
        with torch.no_grad():
            d = ops.DropoutFn.apply(x, p, rng, 1)
            return ops.linear(d, w, b) + ((1.0 - mask) * -10000.0).unsqueeze(1)
    return fwd, bwd, fused_ops, three_pass, byts, keep


def graphed(fn):
    """fn captured once; the returned callable replays it (same launches, no Python or allocator work per call)."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    torch.cuda.synchronize()
    g._keep = out
    return g.replay


def weight_norm_case(dev, n_out, n_in):
    from ytvln import _lib, ops
    n = n_out * n_in
    v, g = torch.randn(n, device=dev) * 0.02, torch.tensor(1.5, device=dev)
    w, dwt, dv, dg, stat = torch.empty_like(v), torch.randn(n, device=dev), torch.empty_like(v), torch.empty((), device=dev), torch.empty(2, device=dev)
    ws = torch.empty(_lib.load().ytvln_weight_norm_workspace_elems(n), device=dev)
    st = ops._stream

    def fwd():
        ops.call("ytvln_weight_norm_fwd_f32", v.data_ptr(), g.data_ptr(), n, w.data_ptr(), None, stat.data_ptr(), ws.data_ptr(), st())

    def bwd():
        ops.call("ytvln_weight_norm_bwd_f32", v.data_ptr(), dwt.data_ptr(), stat.data_ptr(), n, dv.data_ptr(), dg.data_ptr(), ws.data_ptr(), st())
    return fwd, bwd, {"fwd": (8 * n, 12 * n), "bwd": (12 * n, 20 * n)}, (v, g, w, dwt, dv, dg, stat, ws)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heads_cost.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    p = 0.1
    f_fwd, f_bwd, f_ops, f_three, f_bytes, k1 = row_logit_case(dev, 16128, 1024, torch.float32, p)
    b_fwd, b_bwd, _, _, b_bytes, k2 = row_logit_case(dev, 129024, 1024, torch.bfloat16, p)
    w_fwd, w_bwd, w_bytes, k3 = weight_norm_case(dev, 2048, 1024)
    configs = {"row_logit_fwd_f32": f_fwd, "row_logit_fwd_f32_ops": f_ops, "three_pass_fwd_f32": f_three,
               "row_logit_fwd_f32_graph": graphed(f_ops), "three_pass_fwd_f32_graph": graphed(f_three), "row_logit_bwd_f32": f_bwd,
               "row_logit_fwd_bf16": b_fwd, "row_logit_bwd_bf16": b_bwd, "weight_norm_fwd": w_fwd, "weight_norm_bwd": w_bwd}
    t = protocol(dev, configs, a.reps, a.passes)
    torch.cuda.synchronize()
    # the two forward forms computed the same thing
    fused = torch.empty(16128, device=dev)
    f_fwd()
    fused.copy_(k1[5])
    agree = float((fused - f_three().view(-1)).abs().max())
    bytes_of = {"row_logit_fwd_f32": f_bytes["fwd"], "row_logit_bwd_f32": f_bytes["bwd"], "row_logit_fwd_bf16": b_bytes["fwd"],
                "row_logit_bwd_bf16": b_bytes["bwd"], "weight_norm_fwd": w_bytes["fwd"], "weight_norm_bwd": w_bytes["bwd"],
                "three_pass_fwd_f32": (f_bytes["fwd"][0], 3 * 16128 * 1024 * 4 + 5 * 16128 * 4)}
    for k in ("row_logit_fwd_f32_ops", "row_logit_fwd_f32_graph"):
        bytes_of[k] = bytes_of["row_logit_fwd_f32"]
    bytes_of["three_pass_fwd_f32_graph"] = bytes_of["three_pass_fwd_f32"]
    res = {"shapes": {"row_logit_f32": [16128, 1024], "row_logit_bf16": [129024, 1024], "weight_norm": [2048, 1024]}, "dropout_p": p,
           "reps_per_reading": a.reps, "passes": a.passes,
           "protocol": "0.4 s of GEMM before every pass, interleaved, order reversed every pass, min of the passes", "ms": {}}
    for name, v in t.items():
        alg, moved = bytes_of[name]
        res["ms"][name] = {"min": min(v), "passes": v, "spread": max(v) - min(v), "algorithmic_bytes": alg, "bytes_moved": moved,
                           "algorithmic_tb_per_s": alg / (min(v) * 1e-3) / 1e12, "fraction_of_8_tb_per_s": alg / (min(v) * 1e-3) / 1e12 / PEAK_HBM_TBS}
    res["ratio_three_pass_over_fused_fwd_f32_ops"] = res["ms"]["three_pass_fwd_f32"]["min"] / res["ms"]["row_logit_fwd_f32_ops"]["min"]
    res["ratio_three_pass_over_fused_fwd_f32_graph"] = res["ms"]["three_pass_fwd_f32_graph"]["min"] / res["ms"]["row_logit_fwd_f32_graph"]["min"]
    res["max_abs_difference_fused_vs_three_pass"] = agree
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
