#!/usr/bin/env python3
"""Attention backward with stored dS blocks (option ATTN_W1 bit 3) against the recomputing one-wave kernels (ATTN_W1 = 7), site by site.

A measurement, not a gate.  The cfg-2 attention sites at N = 56 with dropout 0.1, each backward launch in isolation, from the same library in
the same process: the co-attention pair (8 heads, d 128, 80 tokens x 288 regions, both directions in one launch per kernel), image
self-attention at 288 regions, text self-attention (12 heads, d 64, 80 tokens).
  * `w7_ms`: dQ kernel (recomputes S, dP and dS, also produces delta) + dK/dV kernel.
  * `w15_ms`: delta pass + dK/dV kernel that also writes its dS blocks + dQ kernel that only contracts them with K; the workspace comes from
    the caching allocator per call, as in a training step.
Protocol of DESIGN.md section 5, shared with tools/grad_clip_cost.py: every pass starts behind 0.4 s of GEMM (warm clocks), the configurations
are interleaved, the order is reversed every pass, min of the passes; a reading is the mean of `--reps` launches between two HIP events.

Every site runs in a child process of its own under `timeout`; the first child that fails, faults or runs out of time ends the run (nothing
more is started on the device).  Writes profiles/attn_stored_ds_cost.json (or --out).

    python tools/attn_stored_ds_cost.py [--reps 20] [--passes 3] [--timeout 120] [--out profiles/attn_stored_ds_cost.json]"""
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

N, P_DROP = 56, 0.1
CASES = {"co_attention_pair": (8, 128, 80, 288, True), "image_self_288": (8, 128, 288, 288, False), "text_self_80": (12, 64, 80, 80, False)}


def worker(case, reps, passes):
    import torch

    from grad_clip_cost import protocol
    from ytvln import _lib, ops
    dev = torch.device("cuda", 0)
    heads, d, Tq, Tk, pair = CASES[case]
    H, scale = heads * d, 1 / math.sqrt(d)
    g = torch.Generator().manual_seed(1)
    st = ops.DropoutState(dev)

    def problem(Tq, Tk, site):
        mk = lambda *s: (torch.randn(s, generator=g) * 0.5).to(dev)          # noqa: E731
        q, kv, dout = mk(N * Tq, H), mk(N * Tk, 2 * H), mk(N * Tq, H)
        mask = torch.zeros(N, Tk, device=dev)
        mask[:, Tk - 3:] = -10000.0
        out, dq, dkv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(kv)
        lse = ops._attn_fwd(q, 0, H, kv, 0, 2 * H, kv, H, 2 * H, mask, out, N, heads, Tq, Tk, d, scale, P_DROP, st.tensor, site)
        delta = torch.empty_like(lse)
        pr = ops._attn_problem(q, 0, H, kv, 0, 2 * H, kv, H, 2 * H, mask, Tq, Tk, P_DROP, site, ctx_in=out, dctx=dout, lse_in=lse, delta=delta,
                               dq=dq, lddq=H, dk=dkv, lddk=2 * H, dv=dkv, dv_off=H, lddv=2 * H)
        return pr, (q, kv, dout, mask, out, dq, dkv, lse, delta)

    pa, keep_a = problem(Tq, Tk, 3)
    pb, keep_b = problem(Tk, Tq, 4) if pair else (None, None)

    def backward(w1):
        def run():
            _lib.set_option("ATTN_W1", w1)
            if pair:
                ops._attn_launch(True, False, pa, pb, N, heads, d, scale, st.tensor)
            else:
                q, kv, dout, mask, out, dq, dkv, lse, _ = keep_a
                ops._attn_bwd(q, 0, H, kv, 0, 2 * H, kv, H, 2 * H, mask, out, dout, lse, dq, 0, H, dkv, 0, 2 * H, dkv, H, 2 * H, N, heads, Tq, Tk, d,
                              scale, P_DROP, st.tensor, 3)
        return run

    _lib.set_option("ATTN_W1", 15)
    elems = int(_lib.load().ytvln_attn_bwd_workspace_elems(N, heads, d, Tq, Tk, Tk if pair else 0, Tq if pair else 0))
    t = protocol(dev, {"w7": backward(7), "w15": backward(15)}, reps, passes)
    torch.cuda.synchronize()
    res = {"case": case, "N": N, "heads": heads, "d": d, "Tq": Tq, "Tk": Tk, "pair": pair, "p_drop": P_DROP, "workspace_bytes": 4 * elems,
           "w7_ms": min(t["w7"]), "w7_passes": t["w7"], "w15_ms": min(t["w15"]), "w15_passes": t["w15"], "w15_over_w7": min(t["w15"]) / min(t["w7"])}
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_stored_ds_cost.json"))
    ap.add_argument("--case")
    a = ap.parse_args()
    if a.case:
        worker(a.case, a.reps, a.passes)
        return 0
    res = {"N": N, "reps_per_reading": a.reps, "passes": a.passes,
           "protocol": "0.4 s of GEMM before every pass, interleaved, order reversed every pass, min of the passes", "cases": []}
    status = 0
    for case in CASES:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(a.reps),
               "--passes", str(a.passes)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            print(f"{case}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            res["stopped_at"] = {"case": case, "exit_status": r.returncode}
            status = 1
            break
        res["cases"].append(json.loads(line[7:]))
        print(line[7:], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return status


if __name__ == "__main__":
    sys.exit(main())
