"""GPU: ytvln_pool_global_rows_f32 / ytvln_expand_records_f32 / ytvln.batch.RecordPool against the numpy statement of
tests/record_pool_ref.py.  Everything is torch.equal except the six trigonometric box columns under `view`: both sides round the same
fp64 value once and device double functions differ from the host's in the last fp64 bits only, so those are held to 2^-24 (one fp32 ulp
below magnitude 1)."""
import functools
import pickle

import numpy as np
import pytest
import torch

from record_pool_ref import expand_records_ref, global_rows_ref, grid_records, mixed_magnitudes, sequential_mean
from test_ragged_pool_gpu import shifted

pytestmark = pytest.mark.gpu

BOXES = 6
GRID = [(F, C) for F in (64, 2048, 6) for C in (21, 1601)]
TRIG = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def case(F, C):
    """(numpy inputs, reference outputs without and with `view` as CPU tensors) of one grid shape; computed once, never modified."""
    inp = grid_records(BOXES, F, C)
    refs = []
    for view in (None, inp[5]):
        ref = expand_records_ref(*inp[:5], BOXES, view)
        assert ref[4] == 0
        refs.append(tuple(torch.from_numpy(a) for a in ref[:4]))
    return inp, refs[0], refs[1]


def same(got, want, trig=False):
    """torch.equal on everything; with `trig` the box columns 5-10 (global rows included) are held to TRIG instead."""
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None)
        if g is None:
            continue
        g = g.cpu()
        assert g.dtype == w.dtype and g.shape == w.shape
        if i == 1 and trig:
            worst = float((g[..., 5:11].double() - w[..., 5:11].double()).abs().max())
            print("box columns 5-10 against the statement: max abs difference", worst)
            assert worst <= TRIG
            assert torch.equal(g[..., :5], w[..., :5]) and torch.equal(g[..., 11], w[..., 11])
        else:
            assert torch.equal(g, w)


def run(inp, dev, view=False, probs=True):
    from ytvln.batch import expand_records, global_rows
    pf, pg, pp, off, idx, turns = (torch.from_numpy(a).to(dev) for a in inp)
    glob = global_rows(pf, off)
    return glob, expand_records(pf, pg, pp if probs else None, glob, off, idx, BOXES, view=turns if view else None)


@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("F,C", GRID)
def test_shape_grid(dev, lib, F, C, view):
    inp, ref, ref_view = case(F, C)
    ns = np.diff(inp[3])
    shown = set(inp[4].reshape(-1).tolist())
    assert {int(ns[p]) for p in shown if p >= 0} == {1, 2, BOXES - 2, BOXES - 1, BOXES, BOXES + 3} and -1 in shown
    assert any(len(set(inp[1][inp[3][p]:inp[3][p + 1], 4])) > 1 for p in shown if p >= 0)     # a frame of two records, two image sizes
    glob, got = run(inp, dev, view)
    assert torch.equal(glob.cpu(), torch.from_numpy(global_rows_ref(inp[0], inp[3])))
    same(got, ref_view if view else ref, trig=view)


@pytest.mark.parametrize("F", [2048, 6])
def test_global_rows_sums_in_row_order(dev, lib, F):
    from ytvln.batch import global_rows
    rs = np.random.RandomState(7)
    x = mixed_magnitudes(rs, (300 + 5, F))
    offsets = np.array([0, 300, 300, 305], np.int64)                    # 300 rows, an empty frame, a short one
    want = global_rows_ref(x, offsets)
    pairwise = x[:300].astype(np.float64).mean(axis=0).astype(np.float32)
    assert np.array_equal(want[0], sequential_mean(x[:300])) and not np.array_equal(pairwise, want[0])     # the test can tell the orders apart
    got = global_rows(torch.from_numpy(x).to(dev), torch.from_numpy(offsets).to(dev))
    assert torch.equal(got.cpu(), torch.from_numpy(want)) and not bool(got[1].any())
    # out=: overwritten whatever it held; pointers one element past a 16-byte boundary
    out = shifted(np.full((3, F), np.nan, np.float32), dev)
    assert global_rows(shifted(x, dev), shifted(offsets, dev), out=out) is out
    assert torch.equal(out.cpu(), torch.from_numpy(want))


@pytest.mark.parametrize("F,C", GRID)
def test_pointers_one_element_past_a_16_byte_boundary(dev, lib, F, C):
    inp, _, ref_view = case(F, C)
    bs, K, frames = inp[4].shape
    R = frames * BOXES
    out = [shifted(np.full(s, np.nan, np.float32), dev) for s in ((bs, K, R, F), (bs, K, R, 12), (bs, K, R, C))]
    out.append(shifted(np.full((bs, K, R), -7, np.int64), dev))
    from ytvln.batch import expand_records, global_rows
    pf, pg, pp, off, idx, view = (shifted(a, dev) for a in inp)
    glob = global_rows(pf, off, out=shifted(np.full((len(inp[3]) - 1, F), np.nan, np.float32), dev))
    got = expand_records(pf, pg, pp, glob, off, idx, BOXES, view=view, out=out)
    assert glob.data_ptr() % 16 == 4 and all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    assert torch.equal(glob.cpu(), torch.from_numpy(global_rows_ref(inp[0], inp[3])))
    same(got, ref_view, trig=True)
    f, bx, pr, m = (t.cpu() for t in out)                               # every element was written: no NaN, no -7, padding exact zeros
    assert bool(((m == 0) | (m == 1)).all()) and not any(bool(torch.isnan(t).any()) for t in (f, bx, pr))
    pad = m == 0
    assert bool(pad.any()) and not bool(f[pad].ne(0).any()) and not bool(pr[pad].ne(0).any()) and not bool(bx[pad][:, :11].ne(0).any())


def test_no_probs(dev, lib):
    inp, ref, _ = case(64, 21)
    _, (f, bx, pr, m) = run(inp, dev, probs=False)
    assert pr is None
    same((f, bx, m), (ref[0], ref[1], ref[3]))


def test_bad_entries_are_padding_and_counted(dev, lib):
    from ytvln.batch import expand_records, global_rows
    inp, ref, _ = case(64, 21)
    pf, pg, pp, off, _ = (torch.from_numpy(a).to(dev) for a in inp[:5])
    glob = global_rows(pf, off)
    idx = inp[4].copy()
    assert idx[1, 2, 1] >= 0 and idx[2, 0, 0] >= 0
    idx[1, 2, 1], idx[2, 0, 0] = len(inp[3]) - 1, -5                    # = pool_frames, and below -1
    want = expand_records_ref(*inp[:4], idx, BOXES)
    assert want[4] == 2
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    got = expand_records(pf, pg, pp, glob, off, torch.from_numpy(idx).to(dev), BOXES, bad=bad)
    same(got, tuple(torch.from_numpy(a) for a in want[:4]))
    assert int(bad) == 2
    bs, K, frames = idx.shape
    for (g, r) in zip(got, ref):                                        # the bad slots are all padding, every other slot as without them
        g, r = g.cpu().view(bs, K, frames, BOXES, -1), r.view(bs, K, frames, BOXES, -1).clone()
        for s in ((1, 2, 1), (2, 0, 0)):
            assert not bool(g[s][..., :11].ne(0).any())
            r[s] = g[s]
        assert torch.equal(g, r)
    expand_records(pf, pg, pp, glob, off, torch.from_numpy(idx).to(dev), BOXES, bad=bad)
    assert int(bad) == 4                                                # accumulates
    # offsets out of order, offsets past the pool, an empty frame: bad as well, their global rows zero, nothing outside the pool is read
    broken = inp[3].copy()
    empty = int(inp[4][1, 0, 0])
    assert empty not in (2, 3, 4, 8, 9, 10, 11)                         # away from the other two breakages
    broken[4], broken[10], broken[empty + 1] = broken[3] - 1, inp[0].shape[0] + 100, broken[empty]
    want = expand_records_ref(*inp[:3], broken, inp[4], BOXES)
    assert want[4] >= 3 and int((inp[4] == empty).sum()) >= 1
    bad.zero_()
    boff = torch.from_numpy(broken).to(dev)
    bglob = global_rows(pf, boff)
    assert torch.equal(bglob.cpu(), torch.from_numpy(global_rows_ref(inp[0], broken))) and not bool(bglob[empty].any())
    got = expand_records(pf, pg, pp, bglob, boff, torch.from_numpy(inp[4]).to(dev), BOXES, bad=bad)
    same(got, tuple(torch.from_numpy(a) for a in want[:4]))
    assert int(bad) == want[4]


def _fill(pool, frames_list):
    pool.reset()
    return [pool.add(i, *fr) for i, fr in enumerate(frames_list)]


def _pool_ref(pool, index, boxes, view):
    ref = expand_records_ref(pool.host_features.numpy(), pool.host_geom.numpy(), pool.host_probs.numpy(), pool.host_offsets.numpy()[:pool.frames + 1],
                             index.numpy(), boxes, view)
    assert ref[4] == 0
    return tuple(torch.from_numpy(a.copy()) for a in ref[:4])


def test_captured_expand_with_view_replays_on_a_refilled_pool(dev, lib):
    from ytvln import synth
    from ytvln.batch import RecordPool
    bs, K, T, frames, boxes, F, C, V = 2, 7, 24, 6, 5, 64, 21, 9
    first = synth.make_record_pool(bs, K, T, frames, boxes, F=F, C=C, seed=21, viewpoints=V)
    second = synth.make_record_pool(bs, K, T, frames, boxes, F=F, C=C, seed=22, viewpoints=V)
    pool = RecordPool(V * (boxes + 3), V, feature_dim=F, num_classes=C, device=dev)
    R = frames * boxes
    out = [torch.full((bs, K, R, w), float("nan"), device=dev) for w in (F, 12, C)] + [torch.full((bs, K, R), -7, dtype=torch.int64, device=dev)]
    _fill(pool, first[0])
    index = RecordPool.index(first[1], frames).to(dev)                  # the static index and view of the captured step
    view = torch.from_numpy(first[4]).to(dev)
    pool.upload()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pool.expand(index, boxes, view=view, out=out)                   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = pool.expand(index, boxes, view=view, out=out)
    assert all(g is o for g, o in zip(got, out))
    graph.replay()
    same(out, _pool_ref(pool, RecordPool.index(first[1], frames), boxes, first[4]), trig=True)
    assert pool.bytes_uploaded == pool.rows * (F + 8 + C) * 4 + (pool.capacity_frames + 1) * 8
    # second batch: pool, offsets, index and view refilled in place, uploaded outside the graph
    _fill(pool, second[0])
    host_index = RecordPool.index(second[1], frames)
    assert not torch.equal(host_index, index.cpu())
    index.copy_(host_index)
    view.copy_(torch.from_numpy(second[4]))
    pool.upload()
    graph.replay()
    same(out, _pool_ref(pool, host_index, boxes, second[4]), trig=True)
    assert int(pool.bad) == 0


def test_end_to_end_on_the_reference_stores_against_the_ragged_pool(dev, lib):
    """reader[...] -> RaggedPool -> expand against reader.records(...) -> RecordPool -> expand, same index: torch.equal, except the
    panorama's columns 5-10: there the ragged side carries the reference's fp32 sin / cos (within 4.4e-8 < 2^-24 of the function on this
    fixture) and the record side the fp64 function rounded once (half an ulp <= 2^-24): 2^-23 between them."""
    from helpers import gold
    from ytvln import features as FR
    from ytvln.batch import RaggedPool, RecordPool
    g = gold("g8_features.npz")
    stores = {k[len("store_"):]: pickle.loads(g[k].tobytes()) for k in g.files if k.startswith("store_")}
    bnb, ytb = FR.BnBFeaturesReader([stores["bnb_old"], stores["bnb_new"]]), FR.YTbFeaturesReader(stores["ytb_new"])
    pano = FR.PanoFeaturesReader(stores["pano"])
    boxes, frames = 8, 3
    queries = [(bnb, ("12-7", "98-3", "12-1")), (bnb, ("98-3",)), (ytb, ("vidB/000031", "vidA/000010")), (ytb, ("vidA/000250",))]
    ragged, record = RaggedPool(200, 8, device=dev), RecordPool(200, 8, device=dev)
    ids = [ragged.add(q, *r[q], max_rows=boxes) for r, q in queries]
    assert ids == [record.add(q, *r.records(q)) for r, q in queries] == [0, 1, 2, 3]
    index = RaggedPool.index([[[0, 1, 2], [3, 2]], [[2, 0], [1]]], frames)
    ragged.upload()
    record.upload()
    a, b = ragged.expand(index, boxes), record.expand(index, boxes)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert int(a[3].sum()) > 0 and int(ragged.bad) == 0 and int(record.bad) == 0
    # the panorama: three viewpoints, each seen under two pairs of headings -- six ragged frames, three record frames
    keys = ["scanA-vp1", "scanA-vp2", "scanB-vp9"]
    turns = [(0.7, -1.9), (-2.4, 0.3)]
    ragged.reset()
    record.reset()
    rid = {(k, t): ragged.add((k, t), *pano[(k, *t)], max_rows=boxes) for k in keys for t in turns}
    vid = {k: record.add(k, *pano.record(k)) for k in keys}
    assert ragged.frames == 6 and record.frames == 3
    walk = [[[(keys[0], turns[0]), (keys[1], turns[1]), (keys[2], turns[0])], [(keys[1], turns[0]), (keys[0], turns[1])]]]
    ragged_index = RaggedPool.index([[[rid[s] for s in o] for o in item] for item in walk], frames)
    record_index = RecordPool.index([[[vid[k] for k, _ in o] for o in item] for item in walk], frames)
    view = torch.zeros(1, 2, frames, 2, dtype=torch.float64)
    for k, o in enumerate(walk[0]):
        for pos, (_, t) in enumerate(o):
            view[0, k, pos] = torch.tensor(t, dtype=torch.float64)
    ragged.upload()
    record.upload()
    assert record.bytes_uploaded < ragged.bytes_uploaded
    a, b = ragged.expand(ragged_index, boxes), record.expand(record_index, boxes, view=view)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert torch.equal(a[1][..., :5], b[1][..., :5]) and torch.equal(a[1][..., 11], b[1][..., 11])
    worst = float((a[1][..., 5:11].double() - b[1][..., 5:11].double()).abs().max())
    print("panorama columns 5-10, ragged (reference fp32 functions) against records: max abs difference", worst)
    assert worst <= 2.0 ** -23 and int(a[3].sum()) > 0 and int(ragged.bad) == 0 and int(record.bad) == 0
