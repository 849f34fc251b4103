"""GPU: the per-score attention bias against fixtures produced by the REAL reference (tools/gen_golden_attn_bias.py -> tests/golden/g20_*):
the connection layer with use_co_attention_mask=True, self-attention with full masks, the whole model with the switch on -- at the bars of
DESIGN.md section 2 (fp32: |d| <= 1e-4 + 1e-4 |ref| on outputs / probabilities / logits, gradient rel-L2 <= 1e-4; bf16-resident: outputs
within 2e-2 relative, gradient norms within 5 %, never bit-equal to fp32) -- and the modes the switch must work with: graph replay, two-stream,
in_batch_pairs, loss_aware_heads, fixed_*_layer, bf16."""
import numpy as np
import pytest
import torch

from helpers import ZERO_DROP, args_ns, cfg_dict, close, gold, rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ALL = dict(ranking=True, traj_judge=True, masked_vision=True, masked_language=True)


def layer_weights(shapes, seed):
    """The generator's recipe: synth.make_weights with the query / key projection weights scaled by 10."""
    from ytvln import synth
    W = synth.make_weights(shapes, seed)
    for k in W:
        if k.endswith("weight") and ("query" in k or "key" in k):
            W[k] = (W[k] * 10.0).astype(np.float32)
    return W


def load_recipe(mod, g, prefix=""):
    W = layer_weights({k: tuple(v.shape) for k, v in mod.state_dict().items()}, int(g[prefix + "seed"]))
    assert list(W) == list(g[prefix + "w_names"])
    assert np.allclose([v.astype(np.float64).sum() for v in W.values()], g[prefix + "w_sum"], rtol=0, atol=1e-9), "weight recipe drifted"
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    return mod


def _cfg(name):
    from ytvln.vilbert import BertConfig
    return BertConfig(**cfg_dict(name, **ZERO_DROP))


def _run_conn(dev, g, gg, cfgname, bf16=False):
    from ytvln import ops
    from ytvln.vilbert import BertConnectionLayer
    layer = load_recipe(BertConnectionLayer(_cfg(cfgname)), g).to(dev).eval()
    layer.biattention.want_probs = True
    t = {k: torch.from_numpy(g[k]).to(dev) for k in ("x1", "x2", "m1", "m2", "co")}
    f1, f2 = torch.from_numpy(gg["f1"]).to(dev), torch.from_numpy(gg["f2"]).to(dev)
    x1, x2 = t["x1"].requires_grad_(), t["x2"].requires_grad_()
    if bf16:
        o1, o2, (p1, p2) = layer(x1.to(BF), t["m1"], x2.to(BF), t["m2"], t["co"], True)
    else:
        o1, o2, (p1, p2) = layer(x1, t["m1"], x2, t["m2"], t["co"], True)
    ((o1.float() * f1).sum() + (o2.float() * f2).sum()).backward()
    return layer, (o1, o2, p1, p2), (x1.grad, x2.grad)


@pytest.mark.parametrize("precision", ["fp32", "fp32x3"])
@pytest.mark.parametrize("case", ["conn_micro", "conn_tiny"])
def test_g20_connection_layer_with_co_attention_mask(dev, lib, case, precision):
    from ytvln import ops
    g = gold(f"g20_attn_bias_{case}.npz")
    gg = gold(f"g20_attn_bias_{case}_grads.npz") if case == "conn_tiny" else g
    prev = ops.get_matmul_precision()
    ops.set_matmul_precision(precision)
    try:
        layer, (o1, o2, p1, p2), (gx1, gx2) = _run_conn(dev, g, gg, "micro.json" if case == "conn_micro" else "tiny_2_2_1.json")
    finally:
        ops.set_matmul_precision(prev)
    close(o1, g["out1"], 1e-4, 1e-4, "layer output 1")
    close(o2, g["out2"], 1e-4, 1e-4, "layer output 2")
    close(p1, g["probs1"], 1e-4, 1e-4, "co-attention probabilities 1 (tokens over regions)")
    close(p2, g["probs2"], 1e-4, 1e-4, "co-attention probabilities 2 (regions over tokens)")
    assert rel_l2(gx1, gg["gx1"]) < 1e-4 and rel_l2(gx2, gg["gx2"]) < 1e-4, (rel_l2(gx1, gg["gx1"]), rel_l2(gx2, gg["gx2"]))
    unused = set(g["unused"])
    for n, p in layer.named_parameters():
        if n in unused:
            assert p.grad is None, n
            continue
        if "grad/" + n in gg.files:
            ref = gg["grad/" + n]
            if n in ("biattention.key1.bias", "biattention.key2.bias"):          # analytically zero (a shift common to all keys): absolute, same scale
                assert float(p.grad.double().norm()) < 1e-4 * float(np.linalg.norm(gg["grad/" + n.replace("key", "query")])), n
                continue
            assert rel_l2(p.grad, ref) < 1e-4, (n, rel_l2(p.grad, ref))
        else:
            if n in ("biattention.key1.bias", "biattention.key2.bias"):
                assert float(p.grad.double().norm()) < 1e-4 * float(gg["gnorm/" + n.replace("key", "query")]), n
                continue
            assert abs(float(p.grad.double().norm()) / float(gg["gnorm/" + n]) - 1) < 1e-4, n
            assert rel_l2(p.grad.reshape(-1)[:64], gg["gslice/" + n]) < 1e-4, (n, rel_l2(p.grad.reshape(-1)[:64], gg["gslice/" + n]))


def test_g20_connection_layer_bf16_resident(dev, lib):
    """The d = 64 case on the bf16-resident path at that path's bars, and not bit-equal to the fp32 result."""
    from ytvln import ops
    g, gg = gold("g20_attn_bias_conn_tiny.npz"), gold("g20_attn_bias_conn_tiny_grads.npz")
    _, (f1, f2, _, _), _ = _run_conn(dev, g, gg, "tiny_2_2_1.json")
    prev = ops.get_matmul_precision()
    ops.set_matmul_precision("bf16")
    try:
        layer, (o1, o2, p1, p2), (gx1, gx2) = _run_conn(dev, g, gg, "tiny_2_2_1.json", bf16=True)
    finally:
        ops.set_matmul_precision(prev)
    assert o1.dtype == BF and o2.dtype == BF
    e = [rel_l2(o1.float(), g["out1"]), rel_l2(o2.float(), g["out2"]), rel_l2(p1, g["probs1"]), rel_l2(p2, g["probs2"])]
    print("g20 bf16 rel-L2 out1 out2 probs1 probs2:", e)
    assert max(e[:2]) < 2e-2 and max(e[2:]) < 2e-2, e
    assert not torch.equal(o1.float(), f1) and not torch.equal(o2.float(), f2), "bf16 run must not be the fp32 run"
    unused = set(g["unused"])
    for n, p in layer.named_parameters():
        if n in unused or "key1.bias" in n or "key2.bias" in n:
            continue
        r = float(p.grad.double().norm()) / float(gg["gnorm/" + n])
        assert abs(r - 1) < 5e-2, (n, r)


@pytest.mark.parametrize("tag", ["t", "v"])
@pytest.mark.parametrize("mname", ["causal", "block", "heads"])
def test_g20_self_attention_with_full_masks(dev, lib, tag, mname):
    from ytvln.vilbert import BertImageSelfAttention, BertSelfAttention
    g = gold("g20_attn_bias_self.npz")
    mod = load_recipe((BertSelfAttention if tag == "t" else BertImageSelfAttention)(_cfg("micro.json")), g, f"{tag}/").to(dev).eval()
    mod.want_probs = True
    x = torch.from_numpy(g[f"{tag}/x"]).to(dev).requires_grad_()
    pre = f"{tag}/{mname}/"
    ctx, probs = mod(x, torch.from_numpy(g[pre + "mask"]).to(dev))
    (ctx * torch.from_numpy(g[f"{tag}/f"]).to(dev)).sum().backward()
    close(ctx, g[pre + "ctx"], 1e-4, 1e-4, "context")
    close(probs, g[pre + "probs"], 1e-4, 1e-4, "probabilities")
    assert rel_l2(x.grad, g[pre + "gx"]) < 1e-4
    for n, p in mod.named_parameters():
        ref = g[pre + "grad/" + n]
        if n == "key.bias":          # analytically zero
            assert float(p.grad.double().norm()) < 1e-4 * float(np.linalg.norm(g[pre + "grad/query.bias"])), n
            continue
        assert rel_l2(p.grad, ref) < 1e-4, (n, rel_l2(p.grad, ref))


# ---- whole model ------------------------------------------------------------------------------------------------------------------------------
def build_lily(dev, cfgname, args, seed, **over):
    from ytvln import synth
    from ytvln.lily import Lily
    from ytvln.vilbert import BertConfig
    cfg = BertConfig(**cfg_dict(cfgname, **{**ZERO_DROP, **over}))
    cfg.args = args
    model = Lily(cfg, dropout_prob=0.0)
    W = synth.make_weights({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    return model.to(dev)


def g0_batch(dev, holes=1):
    from ytvln import synth
    return synth.to_torch(synth.make_batch(bs=2, K=3, T=8, frames=2, boxes=3, F=16, C=11, vocab=97, seed=21, opt_holes=holes, ignore_rank_frac=0.0), dev)


def test_g20_model_with_the_switch_on(dev, lib):
    """encoder.use_co_attention_mask = True on the g0 model and batch against the reference run with the switch on (fixture 3): the four
    logits at 1e-4 + 1e-4 |ref|, the losses at 1e-4; with the switch off the same call reproduces g0 (the mask is ignored)."""
    from ytvln import utils_init as U
    g, g0 = gold("g20_attn_bias_model.npz"), gold("g0_micro.npz")
    args = args_ns(**ALL)
    model = build_lily(dev, "micro.json", args, seed=11).eval()
    batch = g0_batch(dev)
    inputs = list(U.get_model_input(batch))
    inputs[6] = torch.from_numpy(g["co"]).to(dev)
    with torch.no_grad():
        off = model(*inputs)
        for k in off:
            close(off[k], g0["logits/" + k], 1e-4, 1e-4, "switch off: g0 " + k)
        model.bert.encoder.use_co_attention_mask = True
        on = model(*inputs)
    moved = 0.0
    for k in on:
        close(on[k], g["logits/" + k], 1e-4, 1e-4, "switch on: " + k)
        moved = max(moved, float(np.abs(g["logits/" + k] - g0["logits/" + k]).max()))
    assert moved > 2e-3, "the fixture must tell the switch on from off by far more than the bar"
    for task in ("vision", "language", "ranking"):
        _, _, l, _ = U.get_loss_correct(batch, on, task, args, None, True)
        assert abs(float(l) - float(g["loss/" + task])) < 1e-4, (task, float(l), float(g["loss/" + task]))


def _train(dev, mode, steps=5, precision="fp32", two_stream=None, co_seed=5, **over):
    """`steps` training steps on the micro config with the switch on and a seeded {-1, 0, 1} co-attention mask in the batch; returns
    (flattened parameters, last loss)."""
    from ytvln import ops
    from ytvln import utils_init as U
    from ytvln.vilbert_init import get_optimization
    args = args_ns(**ALL)
    args.learning_rate = 1e-3
    batch = list(g0_batch(dev, holes=0))
    bs, K = batch[6].shape[:2]
    Rr, T = batch[3].shape[2], batch[6].shape[2]
    gen = torch.Generator().manual_seed(co_seed)
    batch[11] = torch.randint(-1, 2, (bs, K, Rr, T), generator=gen).to(dev)
    cfgname = "tiny_2_2_1.json" if precision == "bf16" else "micro.json"
    if precision == "bf16":
        from ytvln import synth
        batch = list(synth.to_torch(synth.make_batch(bs=2, K=3, T=16, frames=2, boxes=4, seed=9, ignore_rank_frac=0.0), dev))
        batch[11] = torch.randint(-1, 2, (2, 3, 8, 16), generator=gen).to(dev)
    kw = {k: over.pop(k) for k in ("loss_aware_heads",) if k in over}
    model = build_lily(dev, cfgname, args, seed=11, **over)
    model.train()
    model.bert.encoder.use_co_attention_mask = mode != "off"
    prev_p, prev_ts = ops.get_matmul_precision(), ops.get_two_stream()
    ops.set_matmul_precision(precision)
    if two_stream is not None:
        ops.set_two_stream(two_stream)
    try:
        opt, sched, _, _ = get_optimization(args, model, 10, None)
        for i in range(2):
            U.train_step(model, opt, sched, batch, args, i, all_options=True, **kw)
        if mode == "graph":
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                loss, _ = U.train_step(model, opt, None, batch, args, 0, all_options=True, **kw)
            for i in range(2, steps):
                opt.prepare_replay()
                gr.replay()
                sched.step()
        else:
            for i in range(2, steps):
                loss, _ = U.train_step(model, opt, sched, batch, args, i, all_options=True, **kw)
        torch.cuda.synchronize()
    finally:
        ops.set_matmul_precision(prev_p)
        ops.set_two_stream(prev_ts)
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu(), float(loss)


def test_graph_replay_equals_eager_with_the_switch_on(dev, lib):
    """test_graph_replay_equals_eager's recipe with encoder.use_co_attention_mask = True: the mask is a static input of the captured step."""
    (pe, le), (pg, lg), (po, _) = _train(dev, "eager"), _train(dev, "graph"), _train(dev, "off")
    assert le == lg and torch.equal(pe, pg), float((pe - pg).abs().max())
    assert not torch.equal(pe, po), "the switch must reach the training step"
    assert bool(torch.isfinite(pe).all())


@pytest.mark.parametrize("precision", ["fp32", "fp32x3", "bf16"])
def test_training_with_the_switch_on_two_stream_equals_one_stream(dev, lib, precision):
    (a, la), (b, lb) = _train(dev, "eager", precision=precision, two_stream=True), _train(dev, "eager", precision=precision, two_stream=False)
    assert la == lb and torch.equal(a, b), float((a - b).abs().max())
    off, _ = _train(dev, "off", precision=precision, two_stream=True)
    assert not torch.equal(a, off) and bool(torch.isfinite(a).all())


def test_switch_on_with_loss_aware_heads_and_fixed_layers(dev, lib):
    """loss_aware_heads computes identical losses (logits only for rows with a target); fixed_*_layer runs the lower layers under no_grad:
    both run with the switch on and give finite, different parameters."""
    (a, la), (b, lb) = _train(dev, "eager", steps=3), _train(dev, "eager", steps=3, loss_aware_heads=True)
    # (the loss bar of DESIGN.md section 2; parameters are not compared: AdamW turns rounding-level gradient differences of near-zero gradients
    #  into whole learning-rate steps)
    assert abs(la - lb) < 1e-4 and bool(torch.isfinite(b).all()), (la, lb)
    c, lc = _train(dev, "eager", steps=3, fixed_t_layer=1, fixed_v_layer=1)
    assert np.isfinite(lc) and bool(torch.isfinite(c).all()) and not torch.equal(c, a)


def _dense_encoder_reference(enc, t_emb, v_emb, ext_t, ext_v, ext_co):
    """in_batch_pairs with the switch on, restated with the project's own (already pinned) layers on explicitly expanded inputs: text i against
    image j is row i * b + j and takes TEXT i's mask (vilbert.py:771-778)."""
    b = v_emb.shape[0]
    for l in enc.v_layer[:enc.v_biattention_id[0]]:
        v_emb, _ = l(v_emb, ext_v)
    for l in enc.layer[:enc.t_biattention_id[0]]:
        t_emb, _ = l(t_emb, ext_t)
    rep0 = lambda x: x.unsqueeze(0).expand(b, *x.shape).reshape(b * b, *x.shape[1:])          # noqa: E731  (image side: varies fastest)
    rep1 = lambda x: x.unsqueeze(1).expand(x.shape[0], b, *x.shape[1:]).reshape(b * b, *x.shape[1:])          # noqa: E731
    return enc.c_layer[0](rep0(v_emb).contiguous(), rep0(ext_v).contiguous(), rep1(t_emb).contiguous(), rep1(ext_t).contiguous(),
                          rep1(ext_co).contiguous(), True)[:2]


def test_in_batch_pairs_with_the_switch_on(dev, lib):
    """The encoder's B -> B^2 expansion carries the co-attention mask along (the generator cannot reach it: the reference's local switch sits
    inside the same forward): the encoder's first co-attention output equals the connection layer -- pinned by g20 -- applied to inputs
    expanded by hand, bit for bit, and differs from the run without the mask."""
    from ytvln.vilbert import BertEncoder
    cfg = _cfg("micro.json")
    cfg.in_batch_pairs = True
    torch.manual_seed(3)
    enc = BertEncoder(cfg).to(dev).eval()
    b, T, Rr = 3, 6, 5
    g = torch.Generator().manual_seed(1)
    t_emb = (torch.randn((b, T, cfg.hidden_size), generator=g) * 0.5).to(dev)
    v_emb = (torch.randn((b, Rr, cfg.v_hidden_size), generator=g) * 0.5).to(dev)
    ext_t, ext_v = torch.zeros(b, 1, 1, T, device=dev), torch.zeros(b, 1, 1, Rr, device=dev)
    ext_t[0, ..., T - 2:] = -10000.0
    ext_v[1, ..., Rr - 1:] = -10000.0
    ext_co = (torch.randint(-1, 2, (b, 1, Rr, T), generator=g).float() * 5.0).to(dev)
    with torch.no_grad():
        enc.use_co_attention_mask = True
        all_t, all_v, _ = enc(t_emb, v_emb, ext_t, ext_v, ext_co, output_all_encoded_layers=True)
        want_v, want_t = _dense_encoder_reference(enc, t_emb, v_emb, ext_t, ext_v, ext_co)
        enc.use_co_attention_mask = False
        off_t, off_v, _ = enc(t_emb, v_emb, ext_t, ext_v, ext_co, output_all_encoded_layers=True)
    assert all_t[0].shape[0] == b * b
    assert torch.equal(all_v[0], want_v) and torch.equal(all_t[0], want_t)
    assert not torch.equal(all_t[0], off_t[0])
