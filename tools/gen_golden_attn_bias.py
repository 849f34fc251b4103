"""Generate tests/golden/g20_attn_bias_*.npz by running the REAL reference with per-score attention masks.

TEST INFRASTRUCTURE ONLY; runs where the reference checkout exists (oracle/ref_import.py).  Only data is written.  Usage:

    python tools/gen_golden_attn_bias.py [conn self_attn model]

  g20_attn_bias_conn_micro / _conn_tiny
        the reference's BertConnectionLayer(..., co_attention_mask, use_co_attention_mask=True) in eval mode: micro config sizes of g0
        (N 6, R 5, T 6, 4 heads of 8) and the tiny config (4 heads of 64: a case the bf16-resident path can run) at N 2, R 70, T 45 -- not
        multiples of 32, more than one tile.  Stored: inputs, key masks (padding on both sides at once), the mask, both outputs, both
        probability tensors, and by autograd through the reference the gradients of both inputs and of every parameter for the functional
        sum(out1 * f1) + sum(out2 * f2) with seeded f1, f2.  The tiny case stores parameter gradients as norm + first 64 values, and f1 / f2 and all gradients in g20_attn_bias_conn_tiny_grads.npz
        (no committed file above 1 MiB).
        Mask values: a seeded mix of 0 / +5 / -5 (what BertModel's x 5 makes of a 0 / +-1 mask), N(0,1) draws, -10000 and a few -inf, token 0
        and region 0 kept finite so that every row of both directions keeps a finite key.
  g20_attn_bias_self
        the reference's BertSelfAttention and BertImageSelfAttention (micro config) with [N,1,T,T] masks (causal; block-diagonal "same frame")
        and an [N,h,T,T] mask: context, probabilities, input and parameter gradients.
  g20_attn_bias_model
        the whole reference model (Lily, micro config, the g0 batch and weights) with the co-attention switch ON.  The switch is a local of
        the reference's BertEncoder.forward (vilbert.py:736), so each connection layer's bound `forward` is wrapped at run time to receive
        use_co_attention_mask=True -- the reference's own encoder then runs its own schedule around it; no reference file is edited or copied.
        With the wrapper's flag off the script must reproduce the committed g0 logits exactly, and aborts otherwise.  Stored: the mask
        [rows, R, T] in {-1, 0, 1}, the four logits, the losses.

The weights are synth.make_weights(shapes, seed) with the query / key projection weights scaled by 10 (scores that matter next to the mask);
tests rebuild them from the same recipe, pinned by per-tensor checksums.
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

import gen_golden as G  # noqa: E402
import ref_import  # noqa: E402
from ytvln import synth  # noqa: E402

GOLD = G.GOLD
ALL = dict(ranking=True, traj_judge=True, masked_vision=True, masked_language=True)


def layer_weights(shapes, seed):
    W = synth.make_weights(shapes, seed)
    for k in W:
        if k.endswith("weight") and ("query" in k or "key" in k):
            W[k] = (W[k] * 10.0).astype(np.float32)
    return W


def score_mask(rs, shape, keep_axis):
    """fp32 mask of `shape`; index 0 along the last axis and along `keep_axis` stays finite."""
    b = rs.standard_normal(shape).astype(np.float32)
    u = rs.random_sample(shape)
    b[u < 0.15] = 0.0
    b[(u >= 0.15) & (u < 0.25)] = 5.0
    b[(u >= 0.25) & (u < 0.35)] = -5.0
    b[(u >= 0.35) & (u < 0.45)] = -10000.0
    inf = (u >= 0.45) & (u < 0.50)
    inf[..., 0] = False
    if keep_axis is not None:
        idx = [slice(None)] * len(shape)
        idx[keep_axis] = 0
        inf[tuple(idx)] = False
    b[inf] = -np.inf
    return b


def load(mod, W):
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    return mod.eval()


def conn(R):
    for name, cfgname, N, Rr, T, seed, summarise in (("conn_micro", "micro.json", 6, 5, 6, 31, False), ("conn_tiny", "tiny_2_2_1.json", 2, 70, 45, 32, True)):
        rcfg, _ = G.load_cfg(R, cfgname, **G.ZERO_DROP)
        layer = R.vilbert.BertConnectionLayer(rcfg)
        W = layer_weights({k: tuple(v.shape) for k, v in layer.state_dict().items()}, seed)
        load(layer, W)
        rs = np.random.RandomState(seed)
        x1 = (rs.standard_normal((N, Rr, rcfg.v_hidden_size)) * 0.5).astype(np.float32)
        x2 = (rs.standard_normal((N, T, rcfg.hidden_size)) * 0.5).astype(np.float32)
        m1, m2 = np.zeros((N, 1, 1, Rr), np.float32), np.zeros((N, 1, 1, T), np.float32)
        m1[0, ..., Rr - 2:] = -10000.0
        m2[0, ..., T - 3:] = -10000.0          # pair 0: padding on both sides at the same time
        m2[1, ..., T - 1:] = -10000.0
        co = score_mask(rs, (N, 1, Rr, T), keep_axis=2)
        f1 = rs.standard_normal((N, Rr, rcfg.v_hidden_size)).astype(np.float32)
        f2 = rs.standard_normal((N, T, rcfg.hidden_size)).astype(np.float32)
        t = {k: torch.from_numpy(v) for k, v in dict(x1=x1, x2=x2, m1=m1, m2=m2, co=co, f1=f1, f2=f2).items()}
        t["x1"].requires_grad_(True); t["x2"].requires_grad_(True)
        o1, o2, (p1, p2) = layer(t["x1"], t["m1"], t["x2"], t["m2"], t["co"], True)
        ((o1 * t["f1"]).sum() + (o2 * t["f2"]).sum()).backward()
        for v in (o1, o2, p1, p2, t["x1"].grad, t["x2"].grad):
            if not torch.isfinite(v).all():
                raise SystemExit(f"{name}: the reference produced non-finite values")
        out = dict(x1=x1, x2=x2, m1=m1, m2=m2, co=co, f1=f1, f2=f2, out1=G.np_(o1), out2=G.np_(o2), probs1=G.np_(p1), probs2=G.np_(p2),
                   gx1=G.np_(t["x1"].grad), gx2=G.np_(t["x2"].grad), seed=np.int64(seed),
                   w_names=np.array(list(W)), w_sum=np.array([v.astype(np.float64).sum() for v in W.values()]))
        unused = []
        for n, p in layer.named_parameters():
            if p.grad is None:
                unused.append(n)
            elif summarise:
                out["gnorm/" + n] = np.float64(p.grad.double().norm())
                out["gslice/" + n] = G.np_(p.grad.reshape(-1)[:64])
            else:
                out["grad/" + n] = G.np_(p.grad)
        out["unused"] = np.array(unused)
        path = os.path.join(GOLD, f"g20_attn_bias_{name}.npz")
        if summarise:          # gradients in a file of their own: no committed file above 1 MiB
            gkeys = [k for k in out if k in ("gx1", "gx2", "f1", "f2") or k.startswith(("gnorm/", "gslice/"))]
            gpath = os.path.join(GOLD, f"g20_attn_bias_{name}_grads.npz")
            np.savez_compressed(gpath, **{k: out.pop(k) for k in gkeys})
            assert os.path.getsize(gpath) < (1 << 20), os.path.getsize(gpath)
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
        print(f"g20 {name} ok: {os.path.getsize(path)} bytes, unused {unused}")


def self_attn(R):
    rcfg, _ = G.load_cfg(R, "micro.json", **G.ZERO_DROP)
    out = {}
    for tag, cls, hidden, heads, seed in (("t", R.vilbert.BertSelfAttention, rcfg.hidden_size, rcfg.num_attention_heads, 41),
                                          ("v", R.vilbert.BertImageSelfAttention, rcfg.v_hidden_size, rcfg.v_num_attention_heads, 42)):
        mod = cls(rcfg)
        W = layer_weights({k: tuple(v.shape) for k, v in mod.state_dict().items()}, seed)
        load(mod, W)
        out[f"{tag}/w_names"], out[f"{tag}/w_sum"] = np.array(list(W)), np.array([v.astype(np.float64).sum() for v in W.values()])
        out[f"{tag}/seed"] = np.int64(seed)
        rs = np.random.RandomState(seed)
        N, T = 3, 9
        x = (rs.standard_normal((N, T, hidden)) * 0.5).astype(np.float32)
        f = rs.standard_normal((N, T, hidden)).astype(np.float32)
        causal = np.where(np.tril(np.ones((T, T), bool)), 0.0, -10000.0).astype(np.float32)
        frame = np.arange(T) // 3
        block = np.where(frame[:, None] == frame[None, :], 0.0, -10000.0).astype(np.float32)
        masks = {"causal": np.broadcast_to(causal, (N, 1, T, T)).copy(), "block": np.broadcast_to(block, (N, 1, T, T)).copy(),
                 "heads": score_mask(rs, (N, heads, T, T), keep_axis=None)}
        out[f"{tag}/x"], out[f"{tag}/f"] = x, f
        for mname, m in masks.items():
            xt = torch.from_numpy(x.copy()).requires_grad_(True)
            mod.zero_grad()
            ctx, probs = mod(xt, torch.from_numpy(m))
            (ctx * torch.from_numpy(f)).sum().backward()
            assert torch.isfinite(ctx).all() and torch.isfinite(xt.grad).all()
            pre = f"{tag}/{mname}/"
            out[pre + "mask"], out[pre + "ctx"], out[pre + "probs"], out[pre + "gx"] = m, G.np_(ctx), G.np_(probs), G.np_(xt.grad)
            for n, p in mod.named_parameters():
                out[pre + "grad/" + n] = G.np_(p.grad)
    path = os.path.join(GOLD, "g20_attn_bias_self.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20)
    print(f"g20 self ok: {os.path.getsize(path)} bytes")


def model(R):
    rcfg, _ = G.load_cfg(R, "micro.json", **G.ZERO_DROP)
    args = G.ref_args(**ALL)
    mdl, W, _ = G.build_lily(R, rcfg, args, seed=11)          # the g0 weights
    nb = synth.make_batch(bs=2, K=3, T=8, frames=2, boxes=3, F=16, C=11, vocab=97, seed=21, opt_holes=1, ignore_rank_frac=0.0)     # the g0 batch
    batch = synth.to_torch(nb)
    mdl.eval()
    switch = {"on": False}
    for layer in mdl.bert.encoder.c_layer:          # the reference's own forward, called with the switch the encoder hard-codes to False
        def wrapped(x1, m1, x2, m2, co=None, use=False, _f=layer.forward):
            return _f(x1, m1, x2, m2, co, bool(use or switch["on"]))
        layer.forward = wrapped
    inputs = list(R.utils_init.get_model_input(batch))
    g0 = np.load(os.path.join(GOLD, "g0_micro.npz"))
    with torch.no_grad():
        off = mdl(*inputs)
    for k, v in off.items():
        if not np.array_equal(G.np_(v), g0["logits/" + k]):
            raise SystemExit(f"switch off does not reproduce the committed g0 logits at {k}: the wrapped schedule is not the reference's")
    rows, Rr, T = inputs[1].shape[0], inputs[1].shape[1], inputs[0].shape[1]
    rs = np.random.RandomState(51)
    co = rs.randint(-1, 2, size=(rows, Rr, T)).astype(np.float32)
    inputs[6] = torch.from_numpy(co)
    with torch.no_grad():
        still_off = mdl(*inputs)
        for k, v in still_off.items():
            assert np.array_equal(G.np_(v), g0["logits/" + k]), "switch off must ignore the mask"
        switch["on"] = True
        on = mdl(*inputs)
        total, per = G.ref_losses(R, batch, on, args)
    out = {"co": co}
    for k, v in on.items():
        out["logits/" + k] = G.np_(v)
    if all(np.array_equal(out["logits/" + k], g0["logits/" + k]) for k in on):
        raise SystemExit("switch on changed nothing")
    for k, v in per.items():
        out["loss/" + k] = G.np_(v)
    out["loss/total"] = G.np_(total)
    np.savez_compressed(os.path.join(GOLD, "g20_attn_bias_model.npz"), **out)
    assert os.path.getsize(os.path.join(GOLD, "g20_attn_bias_model.npz")) < (1 << 20)
    print("g20 model ok:", {k: float(v) for k, v in out.items() if k.startswith("loss/")})


if __name__ == "__main__":
    R = ref_import.import_reference()
    for name in sys.argv[1:] or ["conn", "self_attn", "model"]:
        globals()[name](R)
