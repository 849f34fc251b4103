"""GPU: ytvln_expand_ragged_masked / ytvln_expand_records_masked, ytvln.batch.expand_*_masked, the pools' expand_masked,
mask_batch(vision_premasked=True) and the model's bf16 feature input against the statement of tests/pool_masked_ref.py (the existing statement
of the expansion, the oracle's randomize_regions on explicit draws, torch's rounding to bfloat16).  The kernels copy, select and round once, so
every comparison is torch.equal; the one exception is box columns 5-10 of the record pool under `view`, held to 2^-24 as in
test_record_pool_gpu.py."""
import numpy as np
import pytest
import torch

from helpers import ZERO_DROP, cfg_dict
from pool_masked_ref import BIG, BOXES, SHAPES, T_MASK, T_ZERO, make_draws, masked_ref, ragged_case, records_case
from ragged_pool_ref import expand_ragged_ref
from record_pool_ref import expand_records_ref
from test_ragged_pool_gpu import shifted

pytestmark = pytest.mark.gpu

TRIG = 2.0 ** -24
POOLS = ["ragged", "records", "records-view"]
DTYPES = [torch.float32, torch.bfloat16]
BF16_NAN = 0x7FC0


def same(got, want, trig=False):
    """torch.equal on the five outputs; with `trig` the box columns 5-10 are held to TRIG instead."""
    assert len(got) == len(want) == 5
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), i
        if g is None:
            continue
        g = g.cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, (i, g.dtype, w.dtype)
        if i == 1 and trig:
            worst = float((g[..., 5:11].double() - w[..., 5:11].double()).abs().max())
            print("box columns 5-10 against the statement: max abs difference", worst)
            assert worst <= TRIG
            assert torch.equal(g[..., :5], w[..., :5]) and torch.equal(g[..., 11], w[..., 11])
        else:
            assert torch.equal(g, w), i


def case_of(pool, kind, F, C):
    """(boxes, numpy inputs, unmasked statement, draws, the box columns need the trig bar) of one pool and shape."""
    if pool == "ragged":
        return ragged_case(kind, F, C) + (False,)
    return records_case(kind, F, C, pool == "records-view") + (pool == "records-view",)


def fused(pool, inp, boxes, dev, move=None, **kw):
    """The fused expansion of one pool on `inp` (numpy), every input moved to the device by `move`."""
    from ytvln.batch import expand_ragged_masked, expand_records_masked, global_rows
    move = move or (lambda a: torch.from_numpy(a).to(dev))
    if pool == "ragged":
        return expand_ragged_masked(*(move(a) for a in inp), boxes, **kw)
    pf, pg, pp, off, idx, view = (move(a) for a in inp)
    if kw.pop("no_probs", False):
        pp = None
    glob = global_rows(pf, off, out=move(np.full((len(inp[3]) - 1, inp[0].shape[1]), np.nan, np.float32)))
    return expand_records_masked(pf, pg, pp, glob, off, idx, boxes, view=view if pool == "records-view" else None, **kw)


def unfused(pool, inp, boxes, dev):
    """The unchanged composition's first half: expand_ragged / global_rows + expand_records."""
    from ytvln.batch import expand_ragged, expand_records, global_rows
    t = [torch.from_numpy(a).to(dev) for a in inp]
    if pool == "ragged":
        return expand_ragged(*t, boxes)
    pf, pg, pp, off, idx, view = t
    return expand_records(pf, pg, pp, global_rows(pf, off), off, idx, boxes, view=view if pool == "records-view" else None)


# ---- 1: explicit draws against the statement ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind,F,C", SHAPES)
@pytest.mark.parametrize("pool", POOLS)
def test_explicit_draws_against_the_statement(dev, lib, pool, kind, F, C, dtype):
    boxes, inp, ref, p, trig = case_of(pool, kind, F, C)
    got = fused(pool, inp, boxes, dev, p=torch.from_numpy(p).to(dev), feature_dtype=dtype)
    assert got[0].dtype == dtype
    same(got, masked_ref(ref, p, bf16=dtype == torch.bfloat16), trig)


# ---- 2: garbage outputs, shifted pointers ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind,F,C", SHAPES)
@pytest.mark.parametrize("pool", POOLS)
def test_garbage_outputs_and_pointers_one_element_past_a_16_byte_boundary(dev, lib, pool, kind, F, C, dtype):
    boxes, inp, ref, p, trig = case_of(pool, kind, F, C)
    bs, K, frames = inp[4].shape
    R = frames * boxes
    if dtype == torch.bfloat16:
        f = shifted(np.full((bs, K, R, F), BF16_NAN, np.int16), dev).view(torch.bfloat16)
        assert f.data_ptr() % 16 == 2 and bool(torch.isnan(f).all())
    else:
        f = shifted(np.full((bs, K, R, F), np.nan, np.float32), dev)
    out = [f, shifted(np.full((bs, K, R, 12), np.nan, np.float32), dev), shifted(np.full((bs, K, R, C), np.nan, np.float32), dev),
           shifted(np.full((bs, K, R), -7, np.int64), dev), shifted(np.full((bs, K, R), -7, np.int64), dev)]
    got = fused(pool, inp, boxes, dev, move=lambda a: shifted(a, dev), p=shifted(p, dev), feature_dtype=dtype, out=out)
    assert all(g is o for g, o in zip(got, out))
    same(got, masked_ref(ref, p, bf16=dtype == torch.bfloat16), trig)
    f, bx, tg, m, tm = (t.cpu() for t in out)                           # every element was written: no NaN, no -7
    assert not any(bool(torch.isnan(t.float()).any()) for t in (f, bx, tg))
    assert bool(((m == 0) | (m == 1)).all()) and bool(((tm == 0) | (tm == 1)).all())
    pad = m == 0                                                        # padded rows: exact zeros, targets 1 / C, mask 0 whatever their draw
    assert bool(pad.any()) and not bool(f[pad].ne(0).any()) and not bool(bx[pad][:, :11].ne(0).any()) and not bool(tm[pad].any())
    assert bool((tg[pad] == torch.ones(()) / C).all())


# ---- 3: masking off ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("kind,F,C", [SHAPES[0], SHAPES[3], SHAPES[4]])
def test_masking_off(dev, lib, pool, kind, F, C):
    boxes, inp, ref, p, trig = case_of(pool, kind, F, C)
    f, bx, pr, m = unfused(pool, inp, boxes, dev)
    got = fused(pool, inp, boxes, dev, masked_vision=False)
    assert torch.equal(got[0], f) and torch.equal(got[1], bx) and torch.equal(got[3], m)
    assert bool((got[2] == torch.ones((), device=dev) / C).all()) and got[2].shape == pr.shape and not bool(got[4].any()) and got[4].dtype == torch.int64
    same(got, masked_ref(ref, None), trig)                              # = what mask_batch(masked_vision=False) makes of the unfused expansion
    # inference re-ranking: bf16 features, no probabilities
    if pool == "ragged":
        from ytvln.batch import expand_ragged_masked
        pf, pl, _, off, idx = (torch.from_numpy(a).to(dev) for a in inp)
        got = expand_ragged_masked(pf, pl, None, off, idx, boxes, masked_vision=False, feature_dtype=torch.bfloat16)
    else:
        got = fused(pool, inp, boxes, dev, masked_vision=False, feature_dtype=torch.bfloat16, no_probs=True)
    assert got[2] is None and got[4] is None and got[0].dtype == torch.bfloat16
    assert torch.equal(got[0], f.to(torch.bfloat16)) and torch.equal(got[1], bx) and torch.equal(got[3], m)


# ---- 4: production draws are the unfused draws ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("pool", POOLS)
def test_production_draws_are_the_unfused_draws(dev, lib, pool, dtype):
    from ytvln import ops
    from ytvln.batch import randomize_regions
    boxes, inp, ref, _, _ = case_of(pool, "grid", 2048, 1601)
    try:
        ops.DropoutState.manual_seed(77)
        f, bx, pr, m = unfused(pool, inp, boxes, dev)
        f, tg, tm = randomize_regions(f, pr, m)
        want = (f.to(dtype), bx, tg, m, tm)
        ops.DropoutState.manual_seed(77)
        got = fused(pool, inp, boxes, dev, feature_dtype=dtype)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == w.dtype and torch.equal(g, w), i
        assert bool(tm.any()) and not bool(tm[m == 0].any())
        again = fused(pool, inp, boxes, dev, feature_dtype=dtype)        # the device counter advanced: other draws
        assert not torch.equal(again[4], got[4]) and torch.equal(again[3], got[3]) and torch.equal(again[1], got[1])
    finally:
        ops.DropoutState.manual_seed(None)


# ---- 5: bad slots ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("pool", POOLS)
def test_bad_slots_are_padding_and_counted_whatever_their_draws(dev, lib, pool, dtype):
    boxes, inp, _, _, trig = case_of(pool, "grid", 64, 21)
    statement = (lambda off, idx: expand_ragged_ref(*inp[:3], off, idx, boxes)) if pool == "ragged" else \
        (lambda off, idx: expand_records_ref(*inp[:3], off, idx, boxes, inp[5] if pool == "records-view" else None))
    bf16 = dtype == torch.bfloat16
    idx = inp[4].copy()
    assert idx[1, 2, 1] >= 0 and idx[2, 0, 0] >= 0
    idx[1, 2, 1], idx[2, 0, 0] = len(inp[3]) - 1, -5                    # = pool_frames, and below -1
    want = statement(inp[3], idx)
    assert want[4] == 2
    p = make_draws(want[3])                                             # 0.99 on every row of the bad slots
    assert (p.reshape(idx.shape + (boxes,))[1, 2, 1] == np.float32(0.99)).all()
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    args = inp[:4] + (idx,) + inp[5:]
    got = fused(pool, args, boxes, dev, p=torch.from_numpy(p).to(dev), feature_dtype=dtype, bad=bad)
    same(got, masked_ref(want, p, bf16), trig)
    assert int(bad) == 2
    g5 = [t.cpu().view(idx.shape + (boxes, -1)) for t in got]
    for s in ((1, 2, 1), (2, 0, 0)):                                    # all padding
        assert not bool(g5[0][s].ne(0).any()) and not bool(g5[1][s][..., :11].ne(0).any()) and not bool(g5[3][s].any()) and not bool(g5[4][s].any())
        assert bool((g5[2][s] == torch.ones(()) / 21).all())
    fused(pool, args, boxes, dev, p=torch.from_numpy(p).to(dev), feature_dtype=dtype, bad=bad)
    assert int(bad) == 4                                                # accumulates
    # offsets out of order, offsets past the pool and (records) an empty frame
    broken = inp[3].copy()
    empty = int(inp[4][1, 0, 0])
    assert empty not in (2, 3, 4, 8, 9, 10, 11)
    broken[4], broken[10] = broken[3] - 1, inp[0].shape[0] + 100
    if pool != "ragged":
        broken[empty + 1] = broken[empty]
    want = statement(broken, inp[4])
    assert want[4] >= (2 if pool == "ragged" else 3)
    p = make_draws(want[3])
    bad.zero_()
    got = fused(pool, inp[:3] + (broken,) + inp[4:], boxes, dev, p=torch.from_numpy(p).to(dev), feature_dtype=dtype, bad=bad)
    same(got, masked_ref(want, p, bf16), trig)
    assert int(bad) == want[4]


# ---- 6: capture ------------------------------------------------------------------------------------------------------
def _fill(pool, frames_list):
    pool.reset()
    return [pool.add(i, *fr) for i, fr in enumerate(frames_list)]


def _pool_statement(pool, index, boxes, view):
    ref = expand_records_ref(pool.host_features.numpy(), pool.host_geom.numpy(), pool.host_probs.numpy(), pool.host_offsets.numpy()[:pool.frames + 1],
                             index.numpy(), boxes, view)
    assert ref[4] == 0
    return tuple(a.copy() for a in ref[:4])


def _capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()                                                            # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = fn()
    return graph, got


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_captured_expand_masked_replays_on_a_refilled_pool(dev, lib, dtype):
    from ytvln import ops, synth
    from ytvln.batch import RecordPool, expand_records_masked, global_rows
    bs, K, T, frames, boxes, F, C, V = 2, 7, 24, 6, 5, 64, 21, 9
    first = synth.make_record_pool(bs, K, T, frames, boxes, F=F, C=C, seed=21, viewpoints=V)
    second = synth.make_record_pool(bs, K, T, frames, boxes, F=F, C=C, seed=22, viewpoints=V)
    pool = RecordPool(V * (boxes + 3), V, feature_dim=F, num_classes=C, device=dev)
    R = frames * boxes
    bf16 = dtype == torch.bfloat16

    def garbage():
        return [torch.full((bs, K, R, F), float("nan"), device=dev, dtype=dtype)] + [torch.full((bs, K, R, w), float("nan"), device=dev) for w in (12, C)] + \
               [torch.full((bs, K, R), -7, dtype=torch.int64, device=dev) for _ in range(2)]
    out, out_p = garbage(), garbage()
    _fill(pool, first[0])
    index = RecordPool.index(first[1], frames).to(dev)                  # the static index, view and draws of the captured step
    view = torch.from_numpy(first[4]).to(dev)
    p = torch.zeros(bs, K, R, device=dev)
    pool.upload()

    def explicit():
        global_rows(pool.features, pool.offsets, out=pool.global_features)
        return expand_records_masked(pool.features, pool.geom, pool.probs, pool.global_features, pool.offsets, index, boxes, view=view, p=p,
                                     feature_dtype=dtype, out=out_p, bad=pool.bad)
    try:
        ops.DropoutState.manual_seed(5)
        graph_p, got_p = _capture(explicit)
        graph, got = _capture(lambda: pool.expand_masked(index, boxes, view=view, feature_dtype=dtype, out=out))
        assert all(g is o for g, o in zip(got, out)) and all(g is o for g, o in zip(got_p, out_p))
        for batch in (first, second):                                   # second batch: pool, offsets, index, view, draws refilled in place
            _fill(pool, batch[0])
            host_index = RecordPool.index(batch[1], frames)
            index.copy_(host_index)
            view.copy_(torch.from_numpy(batch[4]))
            unmasked = _pool_statement(pool, host_index, boxes, batch[4])
            draws = make_draws(unmasked[3])
            p.copy_(torch.from_numpy(draws))
            pool.upload()
            graph_p.replay()
            same(out_p, masked_ref(unmasked, draws, bf16), trig=True)
            masks = []
            for _ in range(2):                                          # production draws: the device counter advances inside the graph
                graph.replay()
                f, bx, tg, m, tm = (t.cpu() for t in out)
                pr, uf = torch.from_numpy(unmasked[2]), torch.from_numpy(unmasked[0])
                sel = tm.bool()
                assert bool(sel.any()) and torch.equal(tg[sel], pr[sel]) and bool((tg[~sel] == torch.ones(()) / C).all())
                assert torch.equal(m, torch.from_numpy(unmasked[3])) and not bool(tm[m == 0].any())      # no target behind a zero mask
                zeroed = (f.float() == 0).all(-1) & (uf != 0).any(-1)
                assert not bool((zeroed & ~sel).any())                   # only selected rows are zeroed
                keep = ~zeroed
                assert torch.equal(f[keep], (uf.to(dtype))[keep])
                masks.append(tm)
            assert not torch.equal(masks[0], masks[1])
        assert int(pool.bad) == 0
    finally:
        ops.DropoutState.manual_seed(None)


# ---- 7: through the loop ---------------------------------------------------------------------------------------------
def test_through_mask_batch(dev, lib):
    from ytvln import batch as B
    from ytvln import synth
    bs, K, T, frames, boxes, F, C = 2, 7, 24, 6, 5, 64, 21
    frames_list, options, tokens, instr_mask = synth.make_ragged_pool(bs, K, T, frames, boxes, F=F, C=C, seed=31)
    pool = B.RaggedPool(len(frames_list) * boxes, len(frames_list), feature_dim=F, num_classes=C, device=dev)
    pool.reset()
    for i, fr in enumerate(frames_list):
        pool.add(i, *fr, max_rows=boxes)
    host_index = B.RaggedPool.index(options, frames)
    pool.upload()
    batch = synth.to_torch(synth.make_batch(bs=bs, K=K, T=T, frames=frames, boxes=boxes, F=F, C=C, seed=3), dev)
    for dtype in DTYPES:
        f, bx, tg, m, tm = pool.expand_masked(host_index, boxes, feature_dtype=dtype)
        b = list(batch)
        b[1], b[2], b[3], b[4], b[5] = f, bx, m, tg, tm
        b[6], b[7] = torch.from_numpy(tokens).to(dev), torch.from_numpy(instr_mask).to(dev).bool()
        keep = [t.clone() for t in b]
        for masked_vision in (True, False):
            on = B.mask_batch(b, masked_vision=masked_vision, vision_premasked=True)
            for k in (1, 4, 5):
                assert on[k] is b[k] and torch.equal(on[k], keep[k])
            assert on[1].dtype == dtype and bool(on[5].any()) and not bool(on[5][m == 0].any())
            assert bool((on[8] >= 0).any()) and not torch.equal(on[6], keep[6])       # the tokens are still masked
            assert torch.equal(on[8][on[8] >= 0], keep[6][on[8] >= 0])
    # the default is today's function on an unfused batch
    f, bx, pr, m = pool.expand(host_index, boxes)
    b = list(batch)
    b[1], b[2], b[3], b[4] = f, bx, m, pr
    b[6], b[7] = torch.from_numpy(tokens).to(dev), torch.from_numpy(instr_mask).to(dev).bool()
    keep = [t.clone() for t in b]
    on = B.mask_batch(b)
    assert on[1] is b[1] and on[4] is not b[4] and on[4].shape == keep[4].shape
    sel = on[5].bool()
    assert bool(sel.any()) and torch.equal(on[4][sel], keep[4][sel]) and not bool(on[5][keep[3] == 0].any())
    off = B.mask_batch(b, masked_language=False, masked_vision=False)
    assert bool((off[4] == torch.ones((), device=dev) / C).all()) and not bool(off[5].any()) and bool((off[8] == -1).all())


# ---- 8: the model accepts bf16 features bit for bit ------------------------------------------------------------------
def _pretraining_model(dev, dropout):
    from ytvln import synth
    from ytvln.vilbert import BertConfig, BertForMultiModalPreTraining
    cfg = BertConfig(**cfg_dict("tiny_2_2_1.json", **({} if dropout else ZERO_DROP)))          # hidden 256 / 4 heads: head dimension 64
    model = BertForMultiModalPreTraining(cfg)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(shapes, 14).items()})
    return model.to(dev)


@pytest.mark.parametrize("precision,bs,skip,train", [("bf16", 8, None, True), ("bf16", 8, "exact", True), ("bf16", 8, None, False),
                                                     ("fp32", 8, None, True), ("bf16", 3, None, True)],
                         ids=["bf16", "bf16-skip_padding", "bf16-eval", "fp32", "bf16-too-few-rows"])
def test_model_takes_bf16_features_bit_for_bit(dev, lib, precision, bs, skip, train, monkeypatch):
    """bf16 features go into the bf16-resident feature projection as they are (bs = 8: 8 x 10 = 80 rows >= 64, the projection is eligible) and
    are converted to fp32 as before everywhere else (fp32 mode; 3 x 10 = 30 rows): in every case the losses and every parameter gradient equal
    those of the same values passed as fp32, and the eligible cases launch ytvln_cast_f32_bf16 once less."""
    from ytvln import ops, synth
    casts = []
    real_call = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (casts.append(1) if name == "ytvln_cast_f32_bf16" else None, real_call(name, *a))[1])
    model = _pretraining_model(dev, dropout=train)
    model.train(train)
    model.bert.skip_padding = skip
    b = synth.to_torch(synth.make_batch(bs=bs, K=1, T=12, frames=2, boxes=5, seed=24), dev)
    ids, feat, loc, vmask = b[6][:, 0], b[1][:, 0], b[2][:, 0], b[3][:, 0]
    imask, labels = b[7][:, 0], b[8][:, 0]
    img_label, img_target = b[5][:, 0, 1:], b[4][:, 0, 1:]
    nsl = (torch.arange(bs, device=dev) % 2).long()
    assert feat.shape[0] * feat.shape[1] == bs * 10 and (bs * 10 >= 64) == (bs == 8)
    f16 = feat.bfloat16()
    assert not torch.equal(f16.float(), feat)                           # the rounding is not a no-op on these features
    runs = []
    ops.set_matmul_precision(precision)
    try:
        for x in (f16.float(), f16.float(), f16):                        # (the first run also rounds the weights, once: not compared)
            ops.DropoutState.manual_seed(11)
            torch.manual_seed(11)                                       # (the NSP head's nn.Dropout draws from torch's stream)
            model.zero_grad(set_to_none=True)
            del casts[:]
            with torch.set_grad_enabled(train):
                losses = model(ids, x, loc, None, imask, vmask, labels, img_label, img_target, nsl)
                if train:
                    (losses[0] + losses[1] + losses[2]).sum().backward()
            torch.cuda.synchronize()
            runs.append(([l.detach().clone() for l in losses[:3]], {n: q.grad.clone() for n, q in model.named_parameters() if q.grad is not None},
                         len(casts)))
    finally:
        ops.set_matmul_precision("fp32")
        ops.DropoutState.manual_seed(None)
        model.bert.skip_padding = None
    (la, ga, casts_a), (lb, gb, casts_b) = runs[1:]
    assert casts_a - casts_b == (1 if precision == "bf16" and bs == 8 else 0), (casts_a, casts_b)
    assert len(la) == 3 and all(bool(torch.isfinite(l).all()) for l in la)
    for i in range(3):
        assert torch.equal(la[i], lb[i]), (i, float(la[i]), float(lb[i]))
    assert set(ga) == set(gb) and (len(ga) > 0) == train
    bad = [n for n in ga if not torch.equal(ga[n], gb[n])]
    assert not bad, bad[:5]
