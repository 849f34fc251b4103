"""GPU: opt-in activation recomputation (BertEncoder.recompute = "none" | "ffn" | "layer").

Every comparison is bit for bit (torch.equal): the recomputation launches the same deterministic kernels on the same inputs with the dropout
masks of the forward replayed from the recorded (DropoutState, site), so there is no tolerance to choose.  Shapes: configs/tiny_2_2_1.json
(2 text + 2 image layers, one connection layer, 256 wide, FFN 512) on 14 pairs of 16 tokens x 8 regions with holes in both padding masks,
every dropout probability 0.1; configs/micro.json where a second model kind is needed.  The "none" run of a setting is computed once."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT
from helpers import args_ns, cfg_dict
from vltasks_common import make_weights, state_of

pytestmark = pytest.mark.gpu

ALL = dict(ranking=True, traj_judge=True, masked_vision=True, masked_language=True)
RANKING = dict(ranking=True)
N_PAIRS, T, R, INTER = 14, 16, 8, 512
GELU = "ytvln_gelu_fwd_f32"


# ------------------------------------------------------------------------------------------------------------------
# shared inputs, models and runs
# ------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _batch_np():
    """2 samples x 7 options, 16 tokens, 2 frames x 4 regions; three texts and three region sets are cut short (the generator itself fills
    both masks at these sizes)."""
    if "nb" not in _CACHE:
        from ytvln import synth
        nb = synth.make_batch(bs=2, K=7, T=T, frames=2, boxes=4, seed=9, ignore_rank_frac=0.0)
        masks, tmask, tokens, targets = nb[3], nb[5], nb[6].copy(), nb[8]
        for i, k, cut in ((0, 1, 11), (1, 4, 9), (1, 6, 13)):
            tokens[i, k, cut:] = 0
            targets[i, k, cut:] = -1
        nb[6], nb[7] = tokens, tokens > 0
        for i, k, cut in ((0, 2, 6), (1, 0, 5), (1, 5, 7)):
            masks[i, k, cut:] = 0
            tmask[i, k, cut:] = 0
        assert not nb[7].all() and not masks.all() and (targets >= 0).any() and tmask.any()
        _CACHE["nb"] = nb
    return _CACHE["nb"]


def _batch(dev):
    from ytvln import synth
    return synth.to_torch(_batch_np(), dev)


def _load_synth(model, seed=3):
    from ytvln import synth
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    key = ("w", seed, tuple(shapes.items()))
    if key not in _CACHE:
        _CACHE[key] = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in synth.make_weights(shapes, seed).items()}
    model.load_state_dict(_CACHE[key])


def _lily(dev, tier, flags=ALL, **over):
    """Lily on the tiny configuration with identical weights every time; `tier` None leaves the encoder's attribute at its default."""
    from ytvln.lily import Lily
    from ytvln.vilbert import BertConfig
    args = args_ns(**flags)
    args.learning_rate = 1e-3
    cfg = BertConfig(**cfg_dict("tiny_2_2_1.json", **over))
    cfg.args = args
    model = Lily(cfg, dropout_prob=0.1)
    _load_synth(model)
    model.to(dev).train()
    if tier is not None:
        model.bert.encoder.recompute = tier
    return model, args


class _settings:
    """matmul precision, two-stream switch and dropout seed for one run; the defaults come back afterwards."""

    def __init__(self, precision="fp32", two=True, seed=1234):
        self.precision, self.two, self.seed = precision, two, seed

    def __enter__(self):
        from ytvln import ops
        ops.set_matmul_precision(self.precision)
        ops.set_two_stream(self.two)
        ops.DropoutState.manual_seed(self.seed)

    def __exit__(self, *exc):
        from ytvln import ops
        torch.cuda.synchronize()
        ops.set_matmul_precision("fp32")
        ops.set_two_stream(True)
        ops.DropoutState.manual_seed(None)


def _train(dev, tier, precision="fp32", two=True, seed=1234, flags=ALL, **over):
    """Two train steps: the first whole (the optimizer lays out its arenas), the second split into forward + backward and the update, so that
    the gradients -- by then views of the gradient arena, written there directly by the weight-gradient GEMMs -- can be read in between.
    -> (losses, {name: grad or None}, {name: parameter after the second update})."""
    from ytvln import utils_init as U
    from ytvln.optimization import AdamW
    from ytvln.vilbert_init import grouped_parameters
    with _settings(precision, two, seed):
        model, args = _lily(dev, tier, flags, **over)
        opt = AdamW(grouped_parameters(model, 0.01), lr=1e-3)
        batch = _batch(dev)
        l0, _ = U.train_step(model, opt, None, batch, args, 0, all_options=True)
        l1, _ = U.train_step(model, opt, None, batch, args, 1, all_options=True, optimizer_step=False)
        grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}
        opt.step()
        opt.zero_grad()
        torch.cuda.synchronize()
        return (l0.clone(), l1.clone()), grads, {n: p.detach().clone() for n, p in model.named_parameters()}


def _reference(dev, precision="fp32", two=True, **over):
    key = ("none", precision, two, tuple(sorted(over.items())))
    if key not in _CACHE:
        _CACHE[key] = _train(dev, "none", precision, two, **over)
    return _CACHE[key]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _assert_same_run(got, ref, what):
    (gl, gg, gp), (rl, rg, rp) = got, ref
    for a, b in zip(gl, rl):
        assert torch.equal(_bits(a), _bits(b)), (what, "loss", float(a), float(b))
    assert list(gg) == list(rg)
    for n in rg:
        assert (gg[n] is None) == (rg[n] is None), (what, n, "gradient present in one run only")
        if rg[n] is not None:
            assert torch.equal(_bits(gg[n]), _bits(rg[n])), (what, "grad", n, float((gg[n].float() - rg[n].float()).abs().max()))
    for n in rp:
        assert torch.equal(_bits(gp[n]), _bits(rp[n])), (what, "parameter after the step", n, float((gp[n] - rp[n]).abs().max()))


def _count_calls(monkeypatch):
    """Every _lib.call from here on is recorded as (name, args)."""
    from ytvln import _lib, ops
    log, real = [], _lib.call

    def recording(name, *a):
        log.append((name, a))
        return real(name, *a)

    monkeypatch.setattr(_lib, "call", recording)
    monkeypatch.setattr(ops, "call", recording)          # (ops binds the name at import)
    return log


# ------------------------------------------------------------------------------------------------------------------
# 1: the layer tier is exact
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two", [True, False], ids=["two-stream", "one-stream"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_layer_tier_is_bit_identical(dev, lib, precision, two):
    ref = _reference(dev, precision, two)
    assert sum(g is not None for g in ref[1].values()) > 100 and all(torch.isfinite(l) for l in ref[0])
    _assert_same_run(_train(dev, "layer", precision, two), ref, f"layer {precision} two={two}")
    # dropout was live: the same run from another seed draws other masks and lands elsewhere, so a wrong mask in the replay would show
    other = _train(dev, "none", precision, two, seed=4321)
    differing = [n for n, g in ref[1].items() if g is not None and not torch.equal(_bits(g), _bits(other[1][n]))]
    assert len(differing) > 100, len(differing)
    assert any(".c_layer." in n for n in differing) and any(".v_layer." in n for n in differing) and any(".encoder.layer." in n for n in differing)


# ------------------------------------------------------------------------------------------------------------------
# 2: the layer tier saves memory
# ------------------------------------------------------------------------------------------------------------------
def _forward_bytes(dev, tier, flags):
    """Live bytes right after a forward minus live bytes right before it (after one whole step: arenas, caches and streams exist)."""
    from ytvln import utils_init as U
    from ytvln.optimization import AdamW
    from ytvln.vilbert_init import grouped_parameters
    with _settings():
        model, args = _lily(dev, tier, flags)
        opt = AdamW(grouped_parameters(model, 0.01), lr=1e-3)
        batch = _batch(dev)
        U.train_step(model, opt, None, batch, args, 0, all_options=True)
        inputs = U.get_model_input(batch, True)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        out = model(*inputs)
        torch.cuda.synchronize()
        after = torch.cuda.memory_allocated()
        del out
        return after - before


def test_layer_tier_halves_what_a_forward_keeps(dev, lib):
    """What a forward leaves alive for the backward, ranking head only, fp32.  A plain text layer keeps about 12 hidden-state widths per
    row (the layer input, q|k|v = 3, the context, the two LayerNorm sums = 2, the attention output, the GELU pre-activation and the hidden
    of the FFN = 2 + 2 at intermediate = 2 x hidden, plus row statistics), a recomputed one keeps 1: its input.  The five layers are all of
    the encoder; what is left is the two embeddings (a few widths per row, once), the poolers and the ranking head on 14 pooled rows.  So
    the layers shrink twelvefold and the rest stays: one half is the conservative bound.
    Measured on an MI355X: none 13157888 bytes, layer 1768448 (0.134 of none)."""
    none, layer = _forward_bytes(dev, "none", RANKING), _forward_bytes(dev, "layer", RANKING)
    print(f"[recompute] live bytes kept by a forward: none {none}, layer {layer} ({layer / none:.3f} of none)")
    assert layer > 0 and 2 * layer <= none, (none, layer)


# ------------------------------------------------------------------------------------------------------------------
# 3: site accounting
# ------------------------------------------------------------------------------------------------------------------
def test_sites_after_the_encoder_are_unchanged(dev, lib, monkeypatch):
    from ytvln import utils_init as U, vilbert as V
    log = _count_calls(monkeypatch)
    seen = {}
    for tier in ("none", "layer", "ffn"):
        with _settings():
            model, _ = _lily(dev, tier)
            del log[:]
            out = model(*U.get_model_input(_batch(dev), True))
            torch.cuda.synchronize()
            # ytvln_dropout_f32(x, y, n, p, rng, site, stream): Lily's dropout on the fused pooled vector is the first launch of it in a
            # forward, and the first dropout site behind the encoder
            sites = [a[5] for name, a in log if name == "ytvln_dropout_f32"]
            seen[tier] = (V._Runtime.drop._site, sites, out["ranking"].detach().clone())
    counter, sites, ranking = seen["none"]
    # 2 embeddings + 3 sites in each of the 4 single-stream layers + 6 in the connection layer + Lily's own = 21
    assert counter == 21 and sites and sites[-1] == counter, (counter, sites)
    for tier in ("layer", "ffn"):
        assert seen[tier][0] == counter and seen[tier][1] == sites, (tier, seen[tier][:2], counter, sites)
        assert torch.equal(seen[tier][2], ranking), tier          # same pooled vectors, same mask


# ------------------------------------------------------------------------------------------------------------------
# 4: gradient accumulation, plain and data parallel
# ------------------------------------------------------------------------------------------------------------------
def _accumulated_run(dev, tier, wrap=None):
    """Two optimizer steps of two micro-steps each (args.gradient_accumulation_steps = 2) -> every parameter, flat."""
    from ytvln import utils_init as U
    from ytvln.vilbert_init import get_optimization
    with _settings():
        model, args = _lily(dev, tier)
        args.gradient_accumulation_steps = 2
        net = wrap(model) if wrap is not None else model
        opt, sched, _, _ = get_optimization(args, model, 10, None)
        if wrap is not None:
            net.attach(opt)
        batch = _batch(dev)
        for step in range(4):
            U.train_step(net, opt, sched, batch, args, step, all_options=True)
        torch.cuda.synchronize()
        flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu()
        return flat, net


def test_gradient_accumulation_is_bit_identical(dev, lib):
    ref, _ = _accumulated_run(dev, "none")
    got, _ = _accumulated_run(dev, "layer")
    assert torch.equal(_bits(got), _bits(ref)), float((got - ref).abs().max())
    _CACHE["accumulated"] = ref


def _loss_aware_run(dev, tier):
    from ytvln import utils_init as U
    from ytvln.vilbert_init import get_optimization
    with _settings():
        model, args = _lily(dev, tier)
        opt, sched, _, _ = get_optimization(args, model, 10, None)
        batch = _batch(dev)
        losses = [U.train_step(model, opt, sched, batch, args, i, all_options=True, loss_aware_heads=True, capacity_frac=0.5)[0].clone() for i in range(2)]
        torch.cuda.synchronize()
        return losses, torch.cat([p.detach().reshape(-1) for p in model.parameters()])


def test_loss_aware_heads_are_bit_identical(dev, lib):
    (rl, rp), (gl, gp) = _loss_aware_run(dev, "none"), _loss_aware_run(dev, "layer")
    assert all(torch.isfinite(l) for l in rl) and all(torch.equal(a, b) for a, b in zip(gl, rl)), (rl, gl)
    assert torch.equal(_bits(gp), _bits(rp)), float((gp - rp).abs().max())


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                          HSA_ENABLE_IPC_MODE_LEGACY="0")
        os.environ.pop("YTVLN_DP_GRAD_DTYPE", None)
        sys.path.insert(0, os.path.join(ROOT, "youtube-vln_amd"))
        import torch.distributed as dist
        from ytvln import distributed as D
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(0)
        D.init_distributed(backend="gloo", force=True)
        out = {}
        for tier in ("none", "layer"):
            flat, dp = _accumulated_run(dev, tier, wrap=lambda m: D.DataParallel(m, bucket_bytes=1 << 20, collective="rccl", always_exchange=True))
            dp.comm.check_async_error()
            out[tier] = (flat.numpy(), dp._reducer.collectives, len(dp._reducer.buckets))
            dp.close()
        dist.destroy_process_group()
        q.put(("ok", out))
    except Exception as e:      # surface the failure in the parent instead of a bare exit code
        import traceback
        q.put(("error", traceback.format_exc()))
        raise e


def test_gradient_accumulation_under_data_parallel(dev, lib):
    """A one-rank world with the exchange forced on (the collectives run, they are the identity): the bucket hooks fire from the backward
    pass the recomputed node runs inside itself, once per optimizer step, and the parameters are those of the plain run."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_dp_worker, args=(_free_port(), q))
    p.start()
    status, out = q.get(timeout=600)
    p.join(timeout=120)
    assert status == "ok", out
    assert p.exitcode == 0
    (ref, ref_coll, nb), (got, coll, nb2) = out["none"], out["layer"]
    assert nb == nb2 > 1 and ref_coll == coll == 2 * nb, (ref_coll, coll, nb)          # one exchange per optimizer step, in every bucket
    assert np.array_equal(got.view(np.int32), ref.view(np.int32)), float(np.abs(got - ref).max())
    plain = _CACHE["accumulated"] if "accumulated" in _CACHE else _accumulated_run(dev, "none")[0]
    assert np.array_equal(ref.view(np.int32), plain.numpy().view(np.int32)), "the one-rank exchange is the identity"


# ------------------------------------------------------------------------------------------------------------------
# 5: frozen prefix, in_batch_pairs, the downstream-task model
# ------------------------------------------------------------------------------------------------------------------
def test_frozen_prefix_is_exact_and_stays_frozen(dev, lib):
    over = dict(fixed_t_layer=1, fixed_v_layer=1)
    ref = _reference(dev, **over)
    got = _train(dev, "layer", **over)
    _assert_same_run(got, ref, "frozen prefix")
    frozen = [n for n in ref[1] if ".encoder.layer.0." in n or ".encoder.v_layer.0." in n]
    assert len(frozen) == 32, len(frozen)
    for run in (ref, got):          # the layers below the mark run without gradients in either tier; the connection layer above them trains
        assert all(run[1][n] is None for n in frozen)
        assert all(run[1][n] is not None for n in run[1] if ".c_layer.0." in n and ".q_dense" not in n)


def _pairs_run(dev, tier):
    """BertModel with in_batch_pairs (4 texts x 4 images -> 16 rows) under a fixed linear functional of its four outputs."""
    from ytvln import utils_init as U
    from ytvln.vilbert import BertConfig, BertModel
    with _settings():
        model = BertModel(BertConfig(**cfg_dict("tiny_2_2_1.json", in_batch_pairs=True)))
        _load_synth(model, seed=5)
        model.to(dev).train()
        model.encoder.recompute = tier
        ids, feat, loc, seg, imask, vmask = (x[[1, 2, 7, 11]] for x in U.get_model_input(_batch(dev), True)[:6])
        assert not imask.all() and not vmask.all()
        outs = model(ids, feat, loc, seg, imask, vmask)[:4]
        gen = torch.Generator().manual_seed(17)
        loss = sum((o * torch.randn(o.shape, generator=gen).to(dev)).sum() for o in outs)
        loss.backward()
        torch.cuda.synchronize()
        return [o.detach() for o in outs], {n: p.grad for n, p in model.named_parameters()}


def test_in_batch_pairs_is_exact(dev, lib):
    (ro, rg), (go, gg) = _pairs_run(dev, "none"), _pairs_run(dev, "layer")
    assert ro[0].shape[0] == 16 and ro[1].shape[0] == 16
    for a, b in zip(go, ro):
        assert torch.equal(a, b)
    assert sum(g is not None for g in rg.values()) > 100
    for n in rg:
        assert (gg[n] is None) == (rg[n] is None), n
        assert rg[n] is None or torch.equal(gg[n], rg[n]), (n, float((gg[n] - rg[n]).abs().max()))


def _trainable_mask_run(dev, tier):
    """BertModel with use_co_attention_mask and a co_attention_mask that requires grad, under a fixed linear functional of its outputs."""
    from ytvln import utils_init as U
    from ytvln.vilbert import BertConfig, BertModel
    with _settings():
        model = BertModel(BertConfig(**cfg_dict("tiny_2_2_1.json")))
        _load_synth(model, seed=5)
        model.to(dev).train()
        model.encoder.use_co_attention_mask = True
        model.encoder.recompute = tier
        ids, feat, loc, seg, imask, vmask = (x[[1, 2, 7, 11]] for x in U.get_model_input(_batch(dev), True)[:6])
        gen = torch.Generator().manual_seed(19)
        co = (0.3 * torch.randn(4, R, T, generator=gen)).to(dev).requires_grad_(True)
        outs = model(ids, feat, loc, seg, imask, vmask, co)[:4]
        loss = sum((o * torch.randn(o.shape, generator=gen).to(dev)).sum() for o in outs)
        loss.backward()
        torch.cuda.synchronize()
        return co.grad, {n: p.grad for n, p in model.named_parameters()}


def test_trainable_co_attention_mask_keeps_its_gradient(dev, lib):
    (rc, rg), (gc_, gg) = _trainable_mask_run(dev, "none"), _trainable_mask_run(dev, "layer")
    assert rc is not None and float(rc.abs().max()) > 0 and gc_ is not None
    assert torch.equal(gc_, rc), float((gc_ - rc).abs().max())
    for n in rg:
        assert (gg[n] is None) == (rg[n] is None), n
        assert rg[n] is None or torch.equal(gg[n], rg[n]), (n, float((gg[n] - rg[n]).abs().max()))


def _task_run(dev, tier):
    from ytvln import utils_init as U, vl_tasks
    from ytvln.optimization import AdamW
    from ytvln.vilbert import BertConfig, VILBertForVLTasks
    from ytvln.vilbert_init import grouped_parameters
    import warnings
    with _settings():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", FutureWarning)
            model = VILBertForVLTasks(BertConfig(**cfg_dict("micro.json")), 7, dropout_prob=0.1)
        model.load_state_dict(state_of(make_weights(model, 41)))          # (unit-scale weight-norm gains, as the model's own tests use)
        model.to(dev).train()
        model.bert.encoder.recompute = tier
        from ytvln import synth
        nb = synth.make_batch(bs=3, K=2, T=8, frames=2, boxes=3, F=16, C=11, vocab=97, seed=23, ignore_rank_frac=0.0)
        nb[6] = nb[6].copy()
        nb[6][1, 0, 5:] = 0
        nb[7] = nb[6] > 0
        nb[3][2, 1, 4:] = 0
        ids, feat, loc, seg, imask, vmask = U.get_model_input(synth.to_torch(nb, dev), True)[:6]
        assert not imask.all() and not vmask.all()
        target = (torch.rand(ids.shape[0], 7, generator=torch.Generator().manual_seed(3)) < 0.35).float().to(dev)
        batch = (ids, feat, loc, seg, imask.long(), vmask, target)
        opt = AdamW(grouped_parameters(model, 0.01), lr=1e-3)
        losses = [vl_tasks.vl_task_step(model, opt, None, batch, "VL-classifier", args_ns(), step=s)[0].clone() for s in range(2)]
        torch.cuda.synchronize()
        return losses, torch.cat([p.detach().reshape(-1) for p in model.parameters()])


def test_vl_task_step_is_exact(dev, lib):
    (rl, rp), (gl, gp) = _task_run(dev, "none"), _task_run(dev, "layer")
    assert all(torch.isfinite(l) for l in rl) and all(torch.equal(a, b) for a, b in zip(gl, rl)), (rl, gl)
    assert torch.equal(gp, rp), float((gp - rp).abs().max())


# ------------------------------------------------------------------------------------------------------------------
# 6: the GELU recomputation kernel
# ------------------------------------------------------------------------------------------------------------------
SPECIALS = (0.0, 1e-30, -1e-30, 10.0, -10.0, 1e4, -1e4)


def _epilogue_pair(dev):
    """(z, h) of one GEMM with the erf-GELU epilogue, flat: h from ops.linear(x, W, b, "gelu"), z the pre-activation that launch kept for its
    backward.  The first rows of x are value * e_0 against a unit first column of W and a zero bias, so z holds SPECIALS exactly."""
    from ytvln import ops
    gen = torch.Generator().manual_seed(6)
    M, K, N = 40, 24, 128
    x = torch.randn(M, K, generator=gen)
    W = torch.randn(N, K, generator=gen) * 0.6
    W[:, 0] = 1.0
    for i, v in enumerate(SPECIALS):
        x[i] = 0.0
        x[i, 0] = v
    x, W, b = x.to(dev), W.to(dev).requires_grad_(True), torch.zeros(N, device=dev)
    h = ops.linear(x, W, b, "gelu")
    z = h.grad_fn.saved_tensors[2]
    for i, v in enumerate(SPECIALS):
        assert bool((z[i] == v).all()), v
    assert float(z.abs().max()) == 1e4 and float(z[len(SPECIALS):].abs().max()) > 4.0
    return z.detach().reshape(-1).clone(), h.detach().reshape(-1).clone()


def _gelu(z, h, n):
    from ytvln import _lib
    _lib.call(GELU, z.data_ptr() if z is not None else None, h.data_ptr() if h is not None else None, n, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 255, 1023, 4097])
def test_gelu_fwd_equals_the_gemm_epilogue(dev, lib, n):
    if "epilogue" not in _CACHE:
        _CACHE["epilogue"] = _epilogue_pair(dev)
    zs, hs = _CACHE["epilogue"]
    assert zs.numel() >= 4097
    GUARD, MARK = 64, 12345.0
    for z_off in (0, 1):          # element offsets against a 16-byte aligned base: aligned, and 4 bytes past it
        for h_off in (0, 1):
            zbuf = torch.full((n + 8,), float("nan"), device=dev)
            z = zbuf[z_off:z_off + n]
            z.copy_(zs[:n])
            out = torch.full((n + 2 * GUARD + 8,), MARK, device=dev)
            lo = GUARD + h_off
            h = out[lo:lo + n]
            assert zbuf.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
            assert n == 0 or (z.data_ptr() % 16 == 4 * z_off and h.data_ptr() % 16 == 4 * h_off)          # (an empty view has no address)
            _gelu(z, h, n)
            torch.cuda.synchronize()
            assert torch.equal(_bits(h), _bits(hs[:n])), (n, z_off, h_off, float((h - hs[:n]).abs().max()) if n else 0)
            assert bool(torch.isfinite(h).all())
            assert bool((out[:lo] == MARK).all()) and bool((out[lo + n:] == MARK).all()), "written outside [0, n)"
    if n == 0:
        _gelu(None, None, 0)          # an empty tensor has no address
    else:          # in place, and -0.0 (no GEMM output is -0.0: its accumulator starts at +0.0): gelu(-0.0) = -0.0
        z = zs[:n].clone()
        z[0] = -0.0
        _gelu(z, z, n)
        torch.cuda.synchronize()
        assert float(z[0]) == 0.0 and bool(torch.signbit(z[0])) and torch.equal(_bits(z[1:]), _bits(hs[1:n]))


# ------------------------------------------------------------------------------------------------------------------
# 7: the FFN tier is exact and saves what the arithmetic says
# ------------------------------------------------------------------------------------------------------------------
# the FFNs that run with gradients: text layers 0 and 1 and the connection layer's text side on 14 x 16 rows, image layers 0 and 1 and the
# connection layer's image side on 14 x 8 rows; each drops one [rows, 512] fp32 tensor (229 KB and 459 KB: well above the allocator's rounding)
FFN_ROWS = 3 * [N_PAIRS * T] + 3 * [N_PAIRS * R]


def test_ffn_tier_is_bit_identical_and_calls_the_kernel_once_per_ffn(dev, lib, monkeypatch):
    ref = _reference(dev)
    log = _count_calls(monkeypatch)
    _train(dev, "none")
    assert sum(name == GELU for name, _ in log) == 0
    del log[:]
    got = _train(dev, "ffn")
    calls = [a for name, a in log if name == GELU]
    assert sorted(a[2] for a in calls) == sorted(2 * [m * INTER for m in FFN_ROWS]), [a[2] for a in calls]          # two train steps
    _assert_same_run(got, ref, "ffn")


def test_ffn_tier_saves_one_intermediate_per_ffn(dev, lib):
    expected = sum(m * INTER * 4 for m in FFN_ROWS)
    assert min(FFN_ROWS) * INTER * 4 >= 64 << 10
    none, ffn = _forward_bytes(dev, "none", ALL), _forward_bytes(dev, "ffn", ALL)
    # (measured on an MI355X: none 42277888, ffn 40213504; saved 2064384 = the sum, to the byte)
    print(f"[recompute] live bytes kept by a forward: none {none}, ffn {ffn}; saved {none - ffn}, rows x intermediate x 4 summed {expected}")
    assert none - ffn >= 0.95 * expected, (none, ffn, expected)


# ------------------------------------------------------------------------------------------------------------------
# 8: inert when it should be
# ------------------------------------------------------------------------------------------------------------------
def test_tiers_launch_nothing_else_in_eval_and_under_no_grad(dev, lib, monkeypatch):
    from ytvln import utils_init as U
    from ytvln.optimization import AdamW
    from ytvln.vilbert_init import grouped_parameters
    log = _count_calls(monkeypatch)
    names = {}
    for tier in (None, "none", "ffn", "layer"):
        with _settings():
            model, args = _lily(dev, tier)
            inputs = U.get_model_input(_batch(dev), True)
            del log[:]
            model.eval()
            model(*inputs)
            ev = [name for name, _ in log]
            del log[:]
            model.train()
            with torch.no_grad():
                model(*inputs)
            ng = [name for name, _ in log]
            step = None
            if tier in (None, "none"):
                opt = AdamW(grouped_parameters(model, 0.01), lr=1e-3)
                del log[:]
                U.train_step(model, opt, None, _batch(dev), args, 0, all_options=True)
                step = [name for name, _ in log]
            names[tier] = (ev, ng, step)
    assert len(names[None][0]) > 50 and len(names[None][1]) > 50 and len(names[None][2]) > 150
    for tier in ("none", "ffn", "layer"):
        assert names[tier][0] == names[None][0], f"eval forward with recompute = {tier!r}"
        assert names[tier][1] == names[None][1], f"no_grad forward with recompute = {tier!r}"
    assert names["none"][2] == names[None][2], 'a train step with recompute = "none" set explicitly'
    assert GELU not in names[None][2]


# ------------------------------------------------------------------------------------------------------------------
# 9: guards
# ------------------------------------------------------------------------------------------------------------------
def test_guards_raise_and_leave_nothing_installed(dev, lib):
    from ytvln import distributed as D, ops, utils_init as U, vilbert as V
    from ytvln.optimization import AdamW
    from ytvln.vilbert_init import grouped_parameters
    with _settings():
        model, args = _lily(dev, "none")
        enc = model.bert.encoder
        batch = _batch(dev)
        inputs = U.get_model_input(batch, True)
        opt = AdamW(grouped_parameters(model, 0.01), lr=1e-3)
        U.train_step(model, opt, None, batch, args, 0, all_options=True)

        def still_works():
            enc.recompute = "none"
            assert V._Runtime.ffn_recompute is False and ops.TwoStream.active is False
            out = model(*inputs)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(out["ranking"]).all())

        enc.recompute = "rows"
        with pytest.raises(ValueError, match="recompute"):
            model(*inputs)
        still_works()
        enc.recompute = "layer"
        with pytest.raises(NotImplementedError, match="recompute"):
            model.bert(*inputs[:6], output_all_attention_masks=True)
        still_works()
        ops.set_matmul_precision("bf16")
        enc.recompute = "ffn"
        with pytest.raises(NotImplementedError, match="recompute"):
            model(*inputs)
        torch.cuda.synchronize()
        ops.set_matmul_precision("fp32")
        still_works()
        fwd_bwd = lambda backward=None: U.train_step(model, opt, None, batch, args, 0, all_options=True, optimizer_step=False, backward=backward)[0]  # noqa: E731
        for tier in ("ffn", "layer"):
            enc.recompute = tier
            for mode in ("split", "single", "phased"):
                with pytest.raises(NotImplementedError, match="recompute"):
                    D.GraphedTrainStep(model, opt, fwd_bwd, mode=mode)
        still_works()
        U.train_step(model, opt, None, batch, args, 1, all_options=True)          # and an eager step after all of it
        torch.cuda.synchronize()
