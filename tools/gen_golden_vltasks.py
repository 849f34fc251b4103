"""Generate tests/golden/g21_*.npz by running the REAL reference's VILBertForVLTasks / SimpleClassifier (vilbert/vilbert.py:1457-1535).

TEST INFRASTRUCTURE ONLY; runs where the reference checkout exists (oracle/ref_import.py).  Usage:

    python tools/gen_golden_vltasks.py [kats init micro tiny]

Every case is also pushed through an fp64 restatement -- the encoder and the pre-training heads from oracle/vilbert_ref.py, the three new
heads restated here (vltasks_forward) -- and the script aborts when reference and restatement disagree beyond gen_golden.check's defaults,
so a committed fixture certifies reference == restatement == (on the GPU) HIP path.  Only data is written.

  g21_weight_norm_kats  v of [7, 64] and [64, 32], g in {1.5, -0.75}, a seeded dw: w, dv, dg of the reference's weight-normed Linear.
  g21_vltasks_init      torch.manual_seed(1234); VILBertForVLTasks(micro, 7): every key's shape, float64 sum and sum of squares.
  g21_vltasks_micro     micro config, dropout off, num_labels 7, fusion "mul" and (under sum/) "sum": inputs, region mask, weight_g overrides,
                        the 7 outputs, L = sum_i <out_i, c_i> with cotangents(), every gradient of L, the names without a gradient, and the
                        per-tensor parameter norms after three reference AdamW steps (constant lr 4e-5, weight decay 0.01, the grouping of
                        vilbert_init.get_optimization).  Weights: synth.make_weights(seed 41) with weight_g overridden to 1.5 / 0.75.
  g21_vltasks_tiny      tiny config, the summary recipe: outputs sliced, L, per-tensor gradient norms, a 64-element slice of every gradient.
                        Weight gains 13 / 1.5 (G_OVERRIDE_TINY) and the cotangent of vil_prediction noise + (out - b3) / |out - b3| (both stored), so that
                        the gradients of the two weight-norm gains are well-conditioned sums (see loss_and_grads).

SimpleClassifier's inner dropout is 0.5 and the pre-training heads' pooled dropout 0.1 by construction (vilbert.py:1466, 937); the cases run
in training mode and set both to 0 on the modules, like every other dropout.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "youtube-vln_amd"))

import gen_golden as G  # noqa: E402
import ref_import  # noqa: E402
import vilbert_ref as O  # noqa: E402
from ytvln import synth  # noqa: E402

GOLD = G.GOLD
OUT_NAMES = ("vil_prediction", "vil_logit", "vil_binary_prediction", "vision_prediction", "vision_logit", "linguisic_prediction", "linguisic_logit")
G_OVERRIDE = {"vil_prediction.main.0.weight_g": 1.5, "vil_prediction.main.3.weight_g": 0.75}
# the tiny case: about the gains a freshly constructed model of that size has (g = |v|_F of nn.Linear's default init: 13.1 for [512, 256], 1.5 for
# [7, 512]).  With 1.5 on the first layer the pre-activation is its bias (|z - b| = 0.12 against |b| = 0.8) and the gain's gradient vanishes with it.
G_OVERRIDE_TINY = {"vil_prediction.main.0.weight_g": 13.0, "vil_prediction.main.3.weight_g": 1.5}
NUM_LABELS = 7


def vltasks_forward(S, cfg, ids, feat, loc, type_ids, attention_mask, image_attention_mask):
    """VILBertForVLTasks.forward with every dropout off, in the dtype of S (the heads: vilbert.py:1508-1518, 1522-1535)."""
    t, v, pt, pv = O.bert_model(S, cfg, ids, feat, loc, type_ids, attention_mask, image_attention_mask)
    lang, vis, rel = O.pretraining_heads(S, cfg, t, v, pt, pv)
    pooled = pt * pv if cfg.fusion_method == "mul" else pt + pv

    def wn(pre):          # weight_norm(dim=None): one Frobenius norm, one scalar gain
        vv = S[pre + ".weight_v"]
        return vv * (S[pre + ".weight_g"] / vv.norm())

    h = torch.relu(F.linear(pooled, wn("vil_prediction.main.0"), S["vil_prediction.main.0.bias"]))
    vil_prediction = F.linear(h, wn("vil_prediction.main.3"), S["vil_prediction.main.3.bias"])
    vil_logit = O._lin(S, "vil_logit", pooled)
    vision_logit = O._lin(S, "vision_logit", v) + ((1.0 - image_attention_mask.to(v.dtype)) * -10000.0).unsqueeze(2)
    linguisic_logit = O._lin(S, "linguisic_logit", t)
    return vil_prediction, vil_logit, rel, vis, vision_logit, lang, linguisic_logit


def cotangents(shapes, seed):
    """c_i = N(0, 1) / sqrt(numel_i) from numpy RandomState(seed + i): the recipe the GPU tests rebuild."""
    return [(np.random.RandomState(seed + i).standard_normal(tuple(s)) / np.sqrt(max(1, int(np.prod(s))))).astype(np.float32)
            for i, s in enumerate(shapes)]


def checksums(t):
    """float64 sum and sum of squares of the fp32 values, by numpy (pairwise, independent of the thread count)."""
    a = t.detach().numpy().astype(np.float64)
    return float(np.sum(a)), float(np.sum(a * a))


def weights_for(model, seed, gains=None):
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    W = {k: np.asarray(v, dtype=np.float32) for k, v in synth.make_weights(shapes, seed).items()}
    for k, g in (gains or G_OVERRIDE).items():          # make_weights draws every tensor around 0.02: a gain that small (or negative) makes w vanish
        W[k] = np.asarray(g, dtype=np.float32)
    model.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in W.items()})
    return W


def inputs_of(nb, zero_regions):
    b = synth.to_torch(nb)
    ids, feat, loc, seg, imask = b[6][:, 0], b[1][:, 0], b[2][:, 0], b[10][:, 0], b[7][:, 0].long()
    vmask = b[3][:, 0].clone().float()
    for row, n in zero_regions:
        vmask[row, vmask.shape[1] - n:] = 0.0
    return ids, feat, loc, seg, imask, vmask


def build(R, cfgname, fusion, seed, gains=None):
    rcfg, ocfg = G.load_cfg(R, cfgname, fusion_method=fusion, **G.ZERO_DROP)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", FutureWarning)
        model = R.vilbert.VILBertForVLTasks(rcfg, NUM_LABELS, dropout_prob=0.0)
    model.vil_prediction.main[2].p = model.cls.dropout.p = 0.0
    W = weights_for(model, seed, gains)
    model.train()
    return model, ocfg, W


def loss_and_grads(model, ocfg, W, inp, cseed, align_first=False):
    """Reference outputs, L and gradients (left in .grad), all checked against the fp64 restatement.  align_first: the cotangent of
    vil_prediction becomes noise + u / |u| with u = out - b3 (the reference's own output without the last bias, a constant).  The gradient of
    a weight-norm gain is <dw, v> / |v| = (1 / g) <dL/dz, z - b> over the layer's pre-activations z.  With a cotangent unrelated to the
    output that is a cancelling sum of random signs: 1 % of noise on the pooled vectors moves the first gain's gradient by 5 % on average
    and 15 % at worst on the tiny case, so no reduced-precision run can be held to a relative bar on it.  Aligned with the part of the
    output that scales with the gains, the same noise moves it by 0.5 % (1.7 % at worst).  Returns (outs, L, cotangents)."""
    outs = model(*inp)
    cs = cotangents([o.shape for o in outs], cseed)
    if align_first:
        u = (outs[0] - model.vil_prediction.main[3].bias).detach().numpy().astype(np.float64)
        cs[0] = (cs[0] + u / np.linalg.norm(u)).astype(np.float32)
    L = sum((o.double() * torch.from_numpy(c).double()).sum() for o, c in zip(outs, cs))
    model.zero_grad()
    L.backward()
    S = O.trainable({k: torch.as_tensor(np.asarray(v)).double() for k, v in W.items()})
    oouts = vltasks_forward(S, ocfg, *inp)
    oL = sum((o * torch.from_numpy(c).double()).sum() for o, c in zip(oouts, cs))
    oL.backward()
    for n, o, oo in zip(OUT_NAMES, outs, oouts):
        G.check("out/" + n, o, oo)
    G.check("L", L, oL)
    for n, p in model.named_parameters():
        if p.grad is None:
            assert S[n].grad is None, n
        else:
            G.check("grad/" + n, p.grad, S[n].grad)
    return outs, L, cs


def kats(R):
    out = {}
    rs = np.random.RandomState(5)
    for case, (n_out, n_in) in enumerate(((7, 64), (64, 32))):
        v = (rs.standard_normal((n_out, n_in)) / np.sqrt(n_in)).astype(np.float32)
        dw = rs.standard_normal((n_out, n_in)).astype(np.float32)
        for g in (1.5, -0.75):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", FutureWarning)
                lin = R.vilbert.SimpleClassifier(n_in, n_out, 3, 0.0).main[0]
            lin.weight_v.data.copy_(torch.from_numpy(v))
            lin.weight_g.data.fill_(g)
            lin(torch.zeros(1, n_in))                      # the pre-forward hook recomputes lin.weight from (weight_g, weight_v)
            (lin.weight * torch.from_numpy(dw)).sum().backward()
            vd, dwd = torch.from_numpy(v).double().requires_grad_(True), torch.from_numpy(dw).double()
            gd = torch.tensor(g, dtype=torch.float64, requires_grad=True)
            wd = vd * (gd / vd.norm())
            (wd * dwd).sum().backward()
            G.check("w", lin.weight, wd); G.check("dv", lin.weight_v.grad, vd.grad); G.check("dg", lin.weight_g.grad, gd.grad)
            pre = f"case{case}/g{g}/"
            out[pre + "v"], out[pre + "g"], out[pre + "dw"] = v, np.float32(g), dw
            out[pre + "w"], out[pre + "dv"], out[pre + "dg"] = G.np_(lin.weight), G.np_(lin.weight_v.grad), G.np_(lin.weight_g.grad)
    np.savez_compressed(os.path.join(GOLD, "g21_weight_norm_kats.npz"), **out)
    print("g21 kats ok:", len(out) // 6, "cases")


def init(R):
    rcfg, _ = G.load_cfg(R, "micro.json")
    torch.manual_seed(1234)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", FutureWarning)
        sd = R.vilbert.VILBertForVLTasks(rcfg, NUM_LABELS).state_dict()
    out = {"names": np.array(list(sd)), "shapes": np.array([",".join(map(str, v.shape)) for v in sd.values()]),
           "sum": np.array([checksums(v)[0] for v in sd.values()]), "sumsq": np.array([checksums(v)[1] for v in sd.values()])}
    np.savez_compressed(os.path.join(GOLD, "g21_vltasks_init.npz"), **out)
    print("g21 init ok:", len(sd), "keys")


def micro(R):
    nb = synth.make_batch(bs=3, K=1, T=12, frames=2, boxes=5, F=16, C=11, vocab=97, seed=31)
    inp = inputs_of(nb, ((1, 2), (2, 4)))
    out = {"in_%02d" % i: a for i, a in enumerate(nb)}
    out["region_mask"] = inp[5].numpy().copy()
    out["g_names"], out["g_values"] = np.array(list(G_OVERRIDE)), np.array(list(G_OVERRIDE.values()), np.float32)
    for fusion, pre in (("mul", ""), ("sum", "sum/")):
        model, ocfg, W = build(R, "micro.json", fusion, seed=41)
        outs, L, _ = loss_and_grads(model, ocfg, W, inp, cseed=300)
        for n, o in zip(OUT_NAMES, outs):
            out[pre + "out/" + n] = G.np_(o)
        out[pre + "L"] = np.float64(L.item())
        for n, p in model.named_parameters():
            out[pre + "grad/" + n] = G.np_(p.grad) if p.grad is not None else np.zeros(0, np.float32)
        out[pre + "unused"] = np.array([n for n, p in model.named_parameters() if p.grad is None])
        args = G.ref_args(learning_rate=4e-5, weight_decay=0.01, no_scheduler=True)
        opt, sched, _, _ = R.vilbert_init.get_optimization(args, model, 10, None)
        for step in range(3):
            if step:
                loss_and_grads(model, ocfg, {k: G.np_(v) for k, v in model.state_dict().items()}, inp, cseed=300)
            assert abs(sched.get_last_lr()[0] - 4e-5) < 1e-15
            opt.step(); sched.step()
        out[pre + "after3/names"] = np.array([n for n, _ in model.named_parameters()])
        out[pre + "after3/norm"] = np.array([p.double().norm().item() for _, p in model.named_parameters()])
        assert abs(model.vil_prediction.main[0].weight_g.item() - 1.5) > 1e-5          # the 0-d gains moved
        print(f"g21 micro {fusion} ok: L = {L.item():.6f}, unused = {list(out[pre + 'unused'])}")
    np.savez_compressed(os.path.join(GOLD, "g21_vltasks_micro.npz"), **out)


def tiny(R, slices=64):
    nb = synth.make_batch(bs=3, K=1, T=16, frames=2, boxes=4, seed=32)
    inp = inputs_of(nb, ((1, 3),))
    model, ocfg, W = build(R, "tiny_2_2_1.json", "mul", seed=42, gains=G_OVERRIDE_TINY)
    outs, L, cs = loss_and_grads(model, ocfg, W, inp, cseed=400, align_first=True)
    out = {"region_mask": inp[5].numpy().copy(), "L": np.float64(L.item()), "cotangent/vil_prediction": cs[0],
           "g_names": np.array(list(G_OVERRIDE_TINY)), "g_values": np.array(list(G_OVERRIDE_TINY.values()), np.float32)}
    for n, o in zip(OUT_NAMES, outs):
        flat = o.detach().reshape(o.shape[0], -1)
        stride = 1 if o.numel() <= 4096 else max(1, flat.shape[1] // slices)
        out["out/" + n] = G.np_(o) if stride == 1 else G.np_(flat[:, ::stride][:, :slices])
        out["out_stride/" + n] = np.int64(stride)
    names, norms, unused = [], [], []
    for n, p in model.named_parameters():
        if p.grad is None:
            unused.append(n)
            continue
        names.append(n)
        norms.append(p.grad.double().norm().item())
        out["grad_slice/" + n] = G.np_(p.grad.reshape(-1)[:slices])
    out["grad_names"], out["grad_norms"], out["unused"] = np.array(names), np.array(norms), np.array(unused)
    np.savez_compressed(os.path.join(GOLD, "g21_vltasks_tiny.npz"), **out)
    small = {n: v for n, v in zip(names, norms) if v < 1e-3}
    assert all(n.endswith(("key.bias", "key1.bias", "key2.bias")) for n in small), small          # nothing but the identically-zero key biases is tiny
    print(f"g21 tiny ok: L = {L.item():.6f}, {len(names)} gradients, unused = {unused}, gain gradients "
          f"{[v for n, v in zip(names, norms) if n.endswith('weight_g')]}")


if __name__ == "__main__":
    R = ref_import.import_reference()
    for name in sys.argv[1:] or ["kats", "init", "micro", "tiny"]:
        globals()[name](R)
