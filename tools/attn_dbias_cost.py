#!/usr/bin/env python3
"""Cost of the bias-gradient launch (ytvln_attn_dbias_f32 / _bf16) against the attention backward launch of the same problem.

A measurement, not a gate.  The cfg-2 attention problems at N = 56 -- co-attention in both directions (8 heads, d 128, 80 tokens x 288
regions), image self-attention at 288 regions, text self-attention (12 heads, d 64, 80 tokens) -- each with a bias of the three layouts
(`nh` [N,h,Tq,Tk], `n1` [N,1,Tq,Tk], `11` [1,1,Tq,Tk]), in fp32 and on the bf16-resident path, from the same library in the same process:
  * `bwd_ms`: the existing backward entry point with that bias (ytvln_attn_bwd_bias_*: the dQ kernel and the dK/dV kernel, five products).  The
    ABI has no entry that launches the dQ kernel alone, so the whole backward is the yardstick; the dQ kernel is three of its five products.
  * `dbias_ms`: the new launch into a gradient of the bias's layout (two products + one [.., Tq, Tk] fp32 store; `11` adds the workspace pass).
Protocol of DESIGN.md section 5, shared with tools/grad_clip_cost.py: every pass starts behind 0.4 s of GEMM (warm clocks), the configurations
are interleaved, the order is reversed every pass, min of the passes; a reading is the mean of `--reps` launches between two HIP events.

Every (problem, precision) case runs in a child process of its own under `timeout`; the first child that fails, faults or runs out of time
ends the run (nothing more is started on the device).  Writes profiles/attn_dbias_cost.json (or --out).

    python tools/attn_dbias_cost.py [--reps 20] [--passes 3] [--timeout 120] [--out profiles/attn_dbias_cost.json]"""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "youtube-vln_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

N = 56
CASES = {"co_text_over_regions": (8, 128, 80, 288), "co_regions_over_text": (8, 128, 288, 80), "image_self_288": (8, 128, 288, 288),
         "text_self_80": (12, 64, 80, 80)}          # heads, d, Tq, Tk
FORMS = ("nh", "n1", "11")


def worker(case, precision, reps, passes):
    import ctypes

    import torch

    from grad_clip_cost import protocol
    from ytvln import _lib, ops
    dev = torch.device("cuda", 0)
    heads, d, Tq, Tk = CASES[case]
    bf = precision == "bf16"
    H = heads * d
    g = torch.Generator().manual_seed(1)
    mk = lambda *s: (torch.randn(s, generator=g) * 0.5).to(dev).to(torch.bfloat16 if bf else torch.float32)          # noqa: E731
    q, kv, dout = mk(N * Tq, H), mk(N * Tk, 2 * H), mk(N * Tq, H)
    mask = torch.zeros(N, Tk, device=dev)
    mask[:, Tk - 3:] = -10000.0
    out = torch.empty_like(q)
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    scale = 1 / math.sqrt(d)
    configs, keep_alive = {}, []
    for form in FORMS:
        shape = {"nh": (N, heads, Tq, Tk), "n1": (N, 1, Tq, Tk), "11": (1, 1, Tq, Tk)}[form]
        bias = torch.randn(shape, generator=g).to(dev)
        lse = ops._attn_fwd(q, 0, H, kv, 0, 2 * H, kv, H, 2 * H, mask, out, N, heads, Tq, Tk, d, scale, 0.0, None, 0, bias=bias)
        delta = torch.empty_like(lse)
        pr = ops._attn_problem(q, 0, H, kv, 0, 2 * H, kv, H, 2 * H, mask, Tq, Tk, 0.0, 0, ctx_in=out, dctx=dout, lse_in=lse, delta=delta,
                               dq=dq, lddq=H, dk=dkv, lddk=2 * H, dv=dkv, dv_off=H, lddv=2 * H)
        _, brec = ops._attn_bias(bias, N, heads, Tq, Tk)
        grad = torch.empty(shape, device=dev)
        orec = _lib.AttnBias()
        orec.ptr = grad.data_ptr()
        orec.stride_n, orec.stride_h, orec.stride_q, orec.stride_k = ops.attn_bias_strides(grad, N, heads, Tq, Tk)
        need = int(_lib.load().ytvln_attn_dbias_workspace_elems(ctypes.addressof(orec), N, heads, Tq, Tk))
        ws = torch.empty(max(need, 1), device=dev)
        keep_alive += [bias, lse, delta, pr, brec, grad, orec, ws]

        def bwd(pr=pr, brec=brec):
            ops._attn_launch(True, bf, pr, None, N, heads, d, scale, None, ba=brec)

        def dbias(pr=pr, brec=brec, orec=orec, ws=ws, need=need):
            _lib.call("ytvln_attn_dbias_bf16" if bf else "ytvln_attn_dbias_f32", ctypes.addressof(pr), ctypes.addressof(brec),
                      ctypes.addressof(orec), ws.data_ptr(), need, N, heads, d, float(scale), None, ops._stream())

        configs[f"bwd_{form}"], configs[f"dbias_{form}"] = bwd, dbias
    t = protocol(dev, configs, reps, passes)
    torch.cuda.synchronize()
    res = {"case": case, "precision": precision, "N": N, "heads": heads, "d": d, "Tq": Tq, "Tk": Tk, "forms": {}}
    for form in FORMS:
        b, x = t[f"bwd_{form}"], t[f"dbias_{form}"]
        res["forms"][form] = {"bwd_ms": min(b), "bwd_passes": b, "dbias_ms": min(x), "dbias_passes": x, "dbias_over_bwd": min(x) / min(b),
                              "gradient_bytes": 4 * N * heads * Tq * Tk if form == "nh" else 4 * N * Tq * Tk if form == "n1" else 4 * Tq * Tk}
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_dbias_cost.json"))
    ap.add_argument("--case")
    ap.add_argument("--precision")
    a = ap.parse_args()
    if a.case:
        worker(a.case, a.precision, a.reps, a.passes)
        return 0
    res = {"N": N, "reps_per_reading": a.reps, "passes": a.passes,
           "protocol": "0.4 s of GEMM before every pass, interleaved, order reversed every pass, min of the passes",
           "yardstick": "ytvln_attn_bwd_bias_* of the same problem and bias (dQ kernel + dK/dV kernel: five products; the dQ kernel alone has no entry point)",
           "cases": []}
    status = 0
    for precision in ("fp32", "bf16"):
        for case in CASES:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--case", case, "--precision", precision,
                   "--reps", str(a.reps), "--passes", str(a.passes)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
            if r.returncode != 0 or line is None:
                print(f"{case} {precision}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
                res["stopped_at"] = {"case": case, "precision": precision, "exit_status": r.returncode}
                status = 1
                break
            res["cases"].append(json.loads(line[7:]))
            print(line[7:], flush=True)
        if status:
            break
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return status


if __name__ == "__main__":
    sys.exit(main())
