"""Generate tests/golden/g19_swish_kats.npz and g19_swish_micro.npz by running the REAL reference with hidden_act = "swish".

TEST INFRASTRUCTURE ONLY; runs where the reference checkout exists (oracle/ref_import.py).  Usage:

    python tools/gen_golden_swish.py [kats micro tiny]

As in oracle/gen_golden.py every case is also pushed through the oracle restatement (oracle/vilbert_ref.py) and the script aborts when
the two disagree, so a committed fixture certifies reference == oracle == (on the GPU) HIP path.  Only data is written.

  g19_swish_kats   swish/x: a dense sweep of [-20, 20] plus 0, -0.0, +-1e-30, +-87, +-89, +-104, +-1e4, +-3e38 (fp32);
                   swish/y = the reference's swish(x); swish/dy = d sum(swish(x)) / dx by autograd through it.
  g19_swish_micro  the g0 recipe (micro config, all four losses, dropout off: inputs, logits, losses, every gradient, three AdamW steps)
                   with hidden_act = v_hidden_act = "swish"; under mixed/ the case hidden_act = "swish", v_hidden_act = "gelu" (same
                   inputs and weights; logits, losses, gradients) -- the image prediction head follows hidden_act.  The weights are
                   synth.make_weights(seed 11) and are pinned by per-tensor checksums; the AdamW moments after the third step live in
                   g19_swish_micro_adamw.npz (every committed file stays under 1 MiB).
  g19_swish_tiny   the g1 / g2 summary recipe on the tiny config with both activations "swish" (see tiny()): the case the bf16-resident
                   path can run.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "youtube-vln_amd"))

import gen_golden as G  # noqa: E402  (the shared recipe helpers: load_cfg, ref_args, build_lily, check, ref_losses ...)
import ref_import  # noqa: E402
import vilbert_ref as O  # noqa: E402
from ytvln import synth  # noqa: E402

GOLD = G.GOLD
ALL = dict(ranking=True, traj_judge=True, masked_vision=True, masked_language=True)


def kats(R):
    special = [0.0, -0.0, 1e-30, -1e-30, 87.0, -87.0, 89.0, -89.0, 104.0, -104.0, 1e4, -1e4, 3e38, -3e38]
    x = np.concatenate([np.linspace(-20.0, 20.0, 401), np.array(special)]).astype(np.float32)
    xt = torch.from_numpy(x.copy()).requires_grad_(True)
    y = R.vilbert.swish(xt)
    y.sum().backward()
    if not (torch.isfinite(y).all() and torch.isfinite(xt.grad).all()):
        raise SystemExit("reference swish is not finite on the KAT inputs")
    err = G.check("swish", y, O._act("swish", torch.from_numpy(x)), 0.0, 0.0)
    np.savez_compressed(os.path.join(GOLD, "g19_swish_kats.npz"), **{"swish/x": x, "swish/y": G.np_(y), "swish/dy": G.np_(xt.grad)})
    print(f"g19 kats ok: {x.size} values, oracle max diff {err}")


def _forward_and_grads(R, model, batch, args, ocfg, W, out, prefix):
    """Eval-mode logits / losses, then one train-mode backward: everything checked against the oracle and stored under `prefix`."""
    fl = G.flags_of(args)
    model.eval()
    with torch.no_grad():
        outputs = model(*R.utils_init.get_model_input(batch))
        total, per = G.ref_losses(R, batch, outputs, args)
        ids, feat, loc, seg, imask, vmask = O.model_input(batch)
        oo = O.lily_forward(G.state_of(W), ocfg, fl, ids, feat, loc, seg, imask, vmask)
        ototal, oper = O.total_loss(batch, oo, fl)
    for k, v in outputs.items():
        out[prefix + "logits/" + k] = G.np_(v)
        G.check(prefix + "logits/" + k, v, oo[k])
    for k, v in per.items():
        out[prefix + "loss/" + k] = G.np_(v)
        if not k.startswith("correct_"):
            G.check(prefix + "loss/" + k, v, oper[k], 1e-6, 1e-6)
    out[prefix + "loss/total"] = G.np_(total)
    G.check(prefix + "total", total, ototal, 1e-6, 1e-6)


def micro(R):
    out = {}
    args = G.ref_args(**ALL)
    nb = synth.make_batch(bs=2, K=3, T=8, frames=2, boxes=3, F=16, C=11, vocab=97, seed=21, opt_holes=1, ignore_rank_frac=0.0)
    batch = synth.to_torch(nb)
    out.update({"in_%02d" % i: a for i, a in enumerate(nb)})

    # ---- hidden_act = v_hidden_act = "swish": the g0 recipe
    rcfg, ocfg = G.load_cfg(R, "micro.json", hidden_act="swish", v_hidden_act="swish", **G.ZERO_DROP)
    model, W, _ = G.build_lily(R, rcfg, args, seed=11)
    # the weights are synth.make_weights(shapes, seed=11), not stored (size): one checksum per tensor pins the recipe
    out["w_names"], out["w_sum"] = np.array(list(W)), np.array([v.astype(np.float64).sum() for v in W.values()])
    _forward_and_grads(R, model, batch, args, ocfg, W, out, "")
    model.train()
    args.learning_rate = 1e-3
    opt, sched, _, _ = R.vilbert_init.get_optimization(args, model, 10, None)
    S, ost = G.state_of(W), O.AdamWState()
    warm, tot = O.schedule_totals(10, 1, 1)
    for step in range(3):
        total, _ = G.ref_losses(R, batch, model(*R.utils_init.get_model_input(batch)), args)
        total.backward()
        lr_now = sched.get_last_lr()[0]
        assert abs(lr_now - args.learning_rate * O.warmup_linear(step, warm, tot)) < 1e-12
        oloss, _, ograds, _ = O.train_step(S, ocfg, G.flags_of(args), batch, ost, lr_now)
        G.check(f"step{step}.loss", total, oloss, 1e-6, 1e-6)
        if step == 0:
            for n, p in model.named_parameters():
                out["grad/" + n] = G.np_(p.grad) if p.grad is not None else np.zeros(0, np.float32)
                if p.grad is None:
                    assert ograds[n] is None, n
                else:
                    G.check("grad/" + n, p.grad, ograds[n], 1e-6, 1e-4)
            out["unused"] = np.array([n for n, p in model.named_parameters() if p.grad is None])
        out[f"step{step}.loss"], out[f"step{step}.lr"] = G.np_(total), np.float64(lr_now)
        opt.step(); sched.step(); model.zero_grad()
        for n, p in model.named_parameters():
            G.check(f"step{step}.param/" + n, p, S[n], 1e-7, 1e-6)
    moments = {}          # a file of their own: no committed file above 1 MiB
    for n, p in model.named_parameters():
        out["after3/" + n] = G.np_(p)
        if p in opt.state and len(opt.state[p]):
            moments["exp_avg/" + n] = G.np_(opt.state[p]["exp_avg"])
            moments["exp_avg_sq/" + n] = G.np_(opt.state[p]["exp_avg_sq"])
    np.savez_compressed(os.path.join(GOLD, "g19_swish_micro_adamw.npz"), **moments)

    # ---- mixed: text stream and BOTH prediction heads swish (the reference's image head applies hidden_act), image stream gelu
    rcfg, ocfg = G.load_cfg(R, "micro.json", hidden_act="swish", v_hidden_act="gelu", **G.ZERO_DROP)
    args = G.ref_args(**ALL)
    model, W2, _ = G.build_lily(R, rcfg, args, seed=11)
    assert all(np.array_equal(W[k], W2[k]) for k in W)
    _forward_and_grads(R, model, batch, args, ocfg, W, out, "mixed/")
    model.train()
    total, _ = G.ref_losses(R, batch, model(*R.utils_init.get_model_input(batch)), args)
    total.backward()
    _, _, ograds, _ = O.train_step(G.state_of(W), ocfg, G.flags_of(args), batch, O.AdamWState(), 0.0)
    for n, p in model.named_parameters():
        out["mixed/grad/" + n] = G.np_(p.grad) if p.grad is not None else np.zeros(0, np.float32)
        if p.grad is not None:
            G.check("mixed/grad/" + n, p.grad, ograds[n], 1e-6, 1e-4)
    np.savez_compressed(os.path.join(GOLD, "g19_swish_micro.npz"), **out)
    print("g19 micro ok:", {k: float(v) for k, v in out.items() if k.startswith("loss/") or k.startswith("mixed/loss/")})


def tiny(R):
    """tiny 2+2+1 config (hidden 256, head dimension 64: the smallest one the bf16-resident attention kernels take -- the micro config's 8 is
    refused there), all four losses, hidden_act = v_hidden_act = "swish": the summary recipe of g1 / g2 (losses, logits, per-tensor gradient
    norms, parameter checksums after one AdamW step)."""
    rcfg, ocfg = G.load_cfg(R, "tiny_2_2_1.json", hidden_act="swish", v_hidden_act="swish", **G.ZERO_DROP)
    args = G.ref_args(**ALL)
    model, W, _ = G.build_lily(R, rcfg, args, seed=12)
    nb = synth.make_batch(bs=2, K=7, T=16, frames=2, boxes=4, seed=22, ignore_rank_frac=0.0)
    out = {}
    G._summaries(R, model, synth.to_torch(nb), args, ocfg, W, out)
    assert all(np.isfinite(v) for k, v in out.items() if k.startswith("loss/"))
    np.savez_compressed(os.path.join(GOLD, "g19_swish_tiny.npz"), **out)
    print("g19 tiny ok", {k: float(v) for k, v in out.items() if k.startswith("loss/")})


if __name__ == "__main__":
    R = ref_import.import_reference()
    for name in sys.argv[1:] or ["kats", "micro", "tiny"]:
        globals()[name](R)
