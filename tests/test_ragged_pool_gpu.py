"""GPU: ytvln_expand_ragged_f32 / ytvln.batch.expand_ragged / RaggedPool against the numpy statement of tests/ragged_pool_ref.py.
The kernel copies, so every comparison is torch.equal."""
import functools

import numpy as np
import pytest
import torch

from ragged_pool_ref import expand_ragged_ref, grid_pool

pytestmark = pytest.mark.gpu

BOXES = 6
GRID = [(F, C) for F in (64, 2048, 6) for C in (21, 1601)]


@functools.lru_cache(maxsize=None)
def case(F, C):
    """(numpy inputs, reference outputs as CPU tensors) of one grid shape; computed once, never modified."""
    inp = grid_pool(BOXES, F, C)
    ref = expand_ragged_ref(*inp, BOXES)
    assert ref[4] == 0
    return inp, tuple(torch.from_numpy(a) for a in ref[:4])


def same(got, want):
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g.cpu(), w)


def shifted(a, dev):
    """A contiguous device view of `a` that starts one element past a 16-byte boundary."""
    t = torch.from_numpy(a)
    per = 16 // t.element_size()
    buf = torch.empty(t.numel() + per, dtype=t.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
    return v


@pytest.mark.parametrize("F,C", GRID)
def test_shape_grid(dev, lib, F, C):
    from ytvln.batch import expand_ragged
    inp, ref = case(F, C)
    ns = np.diff(inp[3])
    assert {0, 1, 2, BOXES - 1, BOXES, BOXES + 1, BOXES + 3} == set(ns.tolist())
    shown = set(inp[4].reshape(-1).tolist())
    assert {int(ns[p]) for p in shown if p >= 0} == set(ns.tolist()) and -1 in shown        # every kind of frame is shown, and padding
    got = expand_ragged(*(torch.from_numpy(a).to(dev) for a in inp), BOXES)
    same(got, ref)


@pytest.mark.parametrize("F,C", GRID)
def test_pointers_one_element_past_a_16_byte_boundary(dev, lib, F, C):
    from ytvln.batch import expand_ragged
    inp, ref = case(F, C)
    bs, K, frames = inp[4].shape
    R = frames * BOXES
    out = [shifted(np.full(s, np.nan, np.float32), dev) for s in ((bs, K, R, F), (bs, K, R, 12), (bs, K, R, C))]
    out.append(shifted(np.full((bs, K, R), -7, np.int64), dev))
    got = expand_ragged(*(shifted(a, dev) for a in inp), BOXES, out=out)
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    same(got, ref)


def test_no_probs(dev, lib):
    from ytvln.batch import expand_ragged
    inp, ref = case(64, 21)
    pf, pl, pp, off, idx = (torch.from_numpy(a).to(dev) for a in inp)
    f, bx, pr, m = expand_ragged(pf, pl, None, off, idx, BOXES)
    assert pr is None
    same((f, bx, m), (ref[0], ref[1], ref[3]))


@pytest.mark.parametrize("F,C", [(2048, 1601), (6, 21)])
def test_out_tensors_full_of_garbage(dev, lib, F, C):
    from ytvln.batch import expand_ragged
    inp, ref = case(F, C)
    bs, K, frames = inp[4].shape
    R = frames * BOXES
    out = [torch.full((bs, K, R, w), float("nan"), device=dev) for w in (F, 12, C)] + [torch.full((bs, K, R), -7, dtype=torch.int64, device=dev)]
    got = expand_ragged(*(torch.from_numpy(a).to(dev) for a in inp), BOXES, out=out)
    assert all(g is o for g, o in zip(got, out))
    f, bx, pr, m = (t.cpu() for t in out)
    assert bool(((m == 0) | (m == 1)).all())
    pad = m == 0
    assert bool(pad.any()) and not bool(f[pad].ne(0).any()) and not bool(pr[pad].ne(0).any()) and not bool(bx[pad][:, :11].ne(0).any())
    assert not any(bool(torch.isnan(t).any()) for t in (f, bx, pr))
    same(got, ref)


def test_bad_index_entries_are_padding_and_counted(dev, lib):
    from ytvln.batch import expand_ragged
    inp, ref = case(64, 21)
    pf, pl, pp, off, _ = (torch.from_numpy(a).to(dev) for a in inp)
    idx = inp[4].copy()
    assert idx[1, 2, 1] >= 0 and idx[2, 0, 0] >= 0
    idx[1, 2, 1], idx[2, 0, 0] = len(inp[3]) - 1, -5                    # = pool_frames, and below -1
    want = expand_ragged_ref(*inp[:4], idx, BOXES)
    assert want[4] == 2
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    got = expand_ragged(pf, pl, pp, off, torch.from_numpy(idx).to(dev), BOXES, bad=bad)
    same(got, tuple(torch.from_numpy(a) for a in want[:4]))
    assert int(bad) == 2
    bs, K, frames = idx.shape
    for (g, r) in zip(got, ref):                                        # the bad slots are all padding, every other slot as without them
        g, r = g.cpu().view(bs, K, frames, BOXES, -1), r.view(bs, K, frames, BOXES, -1).clone()
        for s in ((1, 2, 1), (2, 0, 0)):
            assert not bool(g[s][..., :11].ne(0).any())
            r[s] = g[s]
        assert torch.equal(g, r)
    expand_ragged(pf, pl, pp, off, torch.from_numpy(idx).to(dev), BOXES, bad=bad)
    assert int(bad) == 4                                                # accumulates
    # offsets out of order / out of range: bad as well, and nothing outside the pool is read
    broken = inp[3].copy()
    broken[4], broken[10] = broken[3] - 1, inp[0].shape[0] + 100
    want = expand_ragged_ref(*inp[:3], broken, inp[4], BOXES)
    assert want[4] >= 2
    bad.zero_()
    got = expand_ragged(pf, pl, pp, torch.from_numpy(broken).to(dev), torch.from_numpy(inp[4]).to(dev), BOXES, bad=bad)
    same(got, tuple(torch.from_numpy(a) for a in want[:4]))
    assert int(bad) == want[4]


def test_agrees_with_expand_options_when_every_frame_is_full(dev, lib):
    from ytvln import batch as B
    g = torch.Generator().manual_seed(5)
    P, boxes, F, C, frames = 23, BOXES, 64, 21, 4
    pf = torch.relu(torch.randn(P, boxes, F, generator=g)).to(dev)
    pb = torch.rand(P, boxes, 12, generator=g).to(dev)
    pp = torch.softmax(torch.randn(P, boxes, C, generator=g), -1).to(dev)
    index = torch.from_numpy(case(F, C)[0][4]).to(dev)
    bs, K, _ = index.shape
    ef, eb, ep, em = B.expand_options(pf, pb, pp, torch.ones(P, boxes, dtype=torch.int64, device=dev), index)
    offsets = torch.arange(P + 1, dtype=torch.int64, device=dev) * boxes
    f, bx, pr, m = B.expand_ragged(pf.view(-1, F), pb[..., :11].reshape(-1, 11).contiguous(), pp.view(-1, C), offsets, index, boxes)
    assert torch.equal(f, ef) and torch.equal(pr, ep) and torch.equal(m, em) and torch.equal(bx[..., :11], eb[..., :11])
    valid = (index >= 0).view(bs, K, frames, 1).expand(bs, K, frames, boxes).reshape(bs, K, frames * boxes)
    assert torch.equal(bx[..., 11][valid], eb[..., 11][valid])
    pos = torch.arange(frames, device=dev).view(1, 1, frames, 1).expand(bs, K, frames, boxes).reshape(bs, K, frames * boxes).float()
    assert bool((~valid).any()) and torch.equal(bx[..., 11][~valid], pos[~valid]) and not bool(eb[..., 11][~valid].ne(0).any())
    assert not bool(m[~valid].any())                                    # the difference sits behind a zero mask


def _fill(pool, frames_list, boxes):
    pool.reset()
    return [pool.add(i, *fr, max_rows=boxes) for i, fr in enumerate(frames_list)]


def _pool_ref(pool, index, boxes):
    ref = expand_ragged_ref(pool.host_features.numpy(), pool.host_locations.numpy(), pool.host_probs.numpy(),
                            pool.host_offsets.numpy()[:pool.frames + 1], index.numpy(), boxes)
    assert ref[4] == 0
    return tuple(torch.from_numpy(a.copy()) for a in ref[:4])


def test_captured_expand_replays_on_a_refilled_pool(dev, lib):
    from ytvln import synth
    from ytvln.batch import RaggedPool
    bs, K, T, frames, boxes, F, C = 2, 7, 24, 6, 5, 64, 21
    first = synth.make_ragged_pool(bs, K, T, frames, boxes, F=F, C=C, seed=21)
    second = synth.make_ragged_pool(bs, K, T, frames, boxes, F=F, C=C, seed=22)
    pool = RaggedPool(len(first[0]) * boxes, len(first[0]), feature_dim=F, num_classes=C, device=dev)
    R = frames * boxes
    out = [torch.full((bs, K, R, w), float("nan"), device=dev) for w in (F, 12, C)] + [torch.full((bs, K, R), -7, dtype=torch.int64, device=dev)]
    _fill(pool, first[0], boxes)
    index = RaggedPool.index(first[1], frames).to(dev)                  # the static index of the captured step
    pool.upload()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pool.expand(index, boxes, out=out)                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = pool.expand(index, boxes, out=out)
    assert all(g is o for g, o in zip(got, out))
    graph.replay()
    same(out, _pool_ref(pool, RaggedPool.index(first[1], frames), boxes))
    assert pool.bytes_uploaded == pool.rows * (F + 11 + C) * 4 + (pool.capacity_frames + 1) * 8
    # second batch: pool, offsets and index refilled in place, uploaded outside the graph
    _fill(pool, second[0], boxes)
    host_index = RaggedPool.index(second[1], frames)
    assert not torch.equal(host_index, index.cpu())
    index.copy_(host_index)
    pool.upload()
    graph.replay()
    same(out, _pool_ref(pool, host_index, boxes))
    assert int(pool.bad) == 0


def test_through_mask_batch(dev, lib):
    """The four outputs dropped into the 16-tuple go through mask_batch unchanged in shape and dtype; with masking disabled they equal the
    host-padded batch."""
    from ytvln import batch as B
    from ytvln import synth
    bs, K, T, frames, boxes, F, C = 2, 7, 24, 6, 5, 64, 21
    frames_list, options, tokens, instr_mask = synth.make_ragged_pool(bs, K, T, frames, boxes, F=F, C=C, seed=31)
    pool = B.RaggedPool(len(frames_list) * boxes, len(frames_list), feature_dim=F, num_classes=C, device=dev)
    _fill(pool, frames_list, boxes)
    host_index = B.RaggedPool.index(options, frames)
    pool.upload()
    f, bx, pr, m = pool.expand(host_index, boxes)
    hf, hb, hp, hm = _pool_ref(pool, host_index, boxes)
    batch = synth.to_torch(synth.make_batch(bs=bs, K=K, T=T, frames=frames, boxes=boxes, F=F, C=C, seed=3), dev)
    b = list(batch)
    b[1], b[2], b[3], b[4], b[6], b[7] = f, bx, m, pr, torch.from_numpy(tokens).to(dev), torch.from_numpy(instr_mask).to(dev).bool()
    off = B.mask_batch(b, masked_language=False, masked_vision=False)
    assert torch.equal(off[1].cpu(), hf) and torch.equal(off[2].cpu(), hb) and torch.equal(off[3].cpu(), hm)
    assert bool((off[4] == torch.ones((), device=dev) / C).all()) and not bool(off[5].any()) and bool((off[8] == -1).all())
    keep = [t.clone() for t in b]
    on = B.mask_batch(b)
    for k in range(16):
        assert on[k].shape == batch[k].shape and on[k].dtype == batch[k].dtype, k
    assert not bool(on[5][keep[3] == 0].any())                          # no MVM target behind a zero mask
    sel = on[5].bool()
    assert torch.equal(on[4][sel], keep[4][sel])
