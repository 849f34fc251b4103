"""CPU: the raw-record frame pool without a device.  The numpy statement of tests/record_pool_ref.py, fed from the decode-only readers
(`records()` / `record()`), against the outputs of the REFERENCE's readers on the same stores (tests/golden/g8_features.npz); the host
logic of ytvln.batch.RecordPool; the argument checks of global_rows / expand_records and of the two C entry points."""
import pickle

import numpy as np
import pytest
import torch

from helpers import gold
from record_pool_ref import expand_records_ref, frame_ref, global_rows_ref, grid_records, sequential_mean

BNB_QUERY, YTB_QUERY, PANO_QUERY = ("12-7", "98-3", "12-1"), ("vidB/000031", "vidA/000010"), ("scanA-vp2", 0.7, -1.9)


@pytest.fixture(scope="module")
def g8():
    g = gold("g8_features.npz")
    return g, {k[len("store_"):]: pickle.loads(g[k].tobytes()) for k in g.files if k.startswith("store_")}


def _readers(stores):
    from ytvln import features as F
    return F.BnBFeaturesReader([stores["bnb_old"], stores["bnb_new"]]), F.YTbFeaturesReader(stores["ytb_new"]), F.PanoFeaturesReader(stores["pano"])


def test_statement_on_decoded_records_reproduces_the_reference_readers(g8):
    g, stores = g8
    bnb, ytb, pano = _readers(stores)
    for name, raw in (("bnb", bnb.records(BNB_QUERY)), ("ytb", ytb.records(YTB_QUERY))):
        assert all(a.dtype == np.float32 for a in raw) and raw[1].shape == (len(raw[0]), 8) and not raw[1][:, 6:].any()
        f, loc, pr = frame_ref(*raw)
        assert all(a.dtype == np.float32 for a in (f, loc, pr))
        assert np.array_equal(f, g[name + "_f"].astype(np.float32))                        # the global row included: the sequential sum
        assert np.array_equal(loc, g[name + "_l"].astype(np.float32))                      # all 11 columns
        assert np.array_equal(pr, g[name + "_p"].astype(np.float32))
    raw = pano.record(PANO_QUERY[0])
    assert all(a.dtype == np.float32 for a in raw) and raw[1][:, 6:].any()
    f, loc, pr = frame_ref(*raw, view=PANO_QUERY[1:])
    want = g["pano_l"].astype(np.float32)
    assert np.array_equal(f, g["pano_f"].astype(np.float32)) and np.array_equal(pr, g["pano_p"].astype(np.float32))
    assert np.array_equal(loc[:, :5], want[:, :5])
    assert np.array_equal(loc[0], want[0])                                                  # the global row: fp64 in the reference as well
    # rows: the reference's fp32 sin / cos against the fp64 function of the same fp32 angle rounded once: half an ulp (<= 2^-24 below 1)
    # for the statement plus the reference's own error, 4.4e-8 < 2^-24 on this fixture
    worst = float(np.abs(loc[1:, 5:].astype(np.float64) - want[1:, 5:].astype(np.float64)).max())
    print("panorama columns 5-10, statement against the reference: max abs difference", worst)
    assert worst <= 2.0 ** -23


def test_records_is_getitem_minus_the_finishing(g8):
    from ytvln import features as F
    g, stores = g8
    bnb, ytb, pano = _readers(stores)
    for reader, query in ((bnb, BNB_QUERY), (ytb, YTB_QUERY)):
        f, geom, pr = reader.records(query)
        rf, rl, rp = reader[query]
        assert np.array_equal(f, rf[1:]) and np.array_equal(pr, rp[1:].astype(np.float32)) and len(geom) == len(rl) - 1
        recs = [F.decode_record(item) for item in reader._items(query)]
        assert np.array_equal(geom[:, :4], np.concatenate([r.boxes for r in recs]))
        assert np.array_equal(geom[:, 4], np.concatenate([np.full(r.num_boxes, r.image_width, np.float32) for r in recs]))
        assert np.array_equal(geom[:, 5], np.concatenate([np.full(r.num_boxes, r.image_height, np.float32) for r in recs]))
        assert len({(r.image_width, r.image_height) for r in recs}) > 1                     # several image sizes inside one frame
    f, geom, pr = pano.record(PANO_QUERY[0])
    rf, rl, rp = pano[PANO_QUERY]
    item = F.decode_pano_record(pickle.loads(stores["pano"][PANO_QUERY[0].encode()]))
    assert np.array_equal(f, rf[1:]) and np.array_equal(pr, rp[1:].astype(np.float32)) and np.array_equal(geom[:, :4], item["boxes"])
    assert np.array_equal(geom[:, 6], item["featureHeading"]) and np.array_equal(geom[:, 7], item["featureElevation"])
    assert set(geom[:, 4]) == {item["image_w"]} and set(geom[:, 5]) == {item["image_h"]}
    with pytest.raises(TypeError):
        pano.record("no-such")
    with pytest.raises(TypeError):
        bnb.records(("no-such-key",))


def _frame(rs, n, F=8, C=5):
    return rs.standard_normal((n, F)).astype(np.float32), rs.uniform(1, 9, (n, 8)).astype(np.float32), rs.uniform(0, 1, (n, C)).astype(np.float32)


def _pool(**kw):
    from ytvln.batch import RecordPool
    args = dict(capacity_rows=20, capacity_frames=6, feature_dim=8, num_classes=5, device=None)
    args.update(kw)
    pool = RecordPool(**args)
    if pool.device is not None:            # a GPU happens to be present: these tests are about the host side only
        pool.device = None
    return pool


def test_record_pool_host_logic(monkeypatch):
    from ytvln.batch import RaggedPool, RecordPool
    rs = np.random.RandomState(0)
    pool = _pool()
    frames = [_frame(rs, n) for n in (3, 1, 5)]
    assert [pool.add(("vp", i), *fr) for i, fr in enumerate(frames)] == [0, 1, 2] and pool.frames == 3 and pool.rows == 9
    assert pool.host_offsets[:4].tolist() == [0, 3, 4, 9]
    for (f, geom, pr), a, b in zip(frames, (0, 3, 4), (3, 4, 9)):
        assert torch.equal(pool.host_features[a:b], torch.from_numpy(f)) and torch.equal(pool.host_geom[a:b], torch.from_numpy(geom))
        assert torch.equal(pool.host_probs[a:b], torch.from_numpy(pr))
    before = [t.clone() for t in (pool.host_features, pool.host_geom, pool.host_probs, pool.host_offsets)]
    assert pool.add(("vp", 1), *_frame(rs, 4)) == 1 and pool.frames == 3 and pool.rows == 9       # dedupe by key: nothing is copied
    assert all(torch.equal(t, b) for t, b in zip((pool.host_features, pool.host_geom, pool.host_probs, pool.host_offsets), before))
    with pytest.raises(ValueError, match="empty"):
        pool.add("nothing", *_frame(rs, 0))
    assert pool.frames == 3 and pool.rows == 9
    with pytest.raises(TypeError):
        pool.add("cut", *_frame(rs, 2), max_rows=1)                     # all rows are shipped: the mean runs over every region
    with pytest.raises(ValueError, match="geom"):
        pool.add("narrow", frames[0][0], frames[0][1][:, :6], frames[0][2])
    with pytest.raises(ValueError, match="probs"):
        pool.add("no probs", frames[0][0], frames[0][1])
    assert pool.frames == 3 and pool.rows == 9
    assert RecordPool.index is RaggedPool.index                         # one helper
    assert RecordPool.index([[[0, 1, 2, 3], [2]]], 3).tolist() == [[[0, 1, 2], [2, -1, -1]]]
    with pytest.raises(RuntimeError, match="GPU"):
        pool.upload()
    with pytest.raises(RuntimeError, match="GPU"):
        pool.expand(torch.zeros(1, 1, 1, dtype=torch.int64), 4)
    # upload() itself, with the device copies replaced by host ones
    pool.device = torch.device("cpu")
    pool.features, pool.geom, pool.probs = (torch.zeros_like(t) for t in (pool.host_features, pool.host_geom, pool.host_probs))
    pool.offsets = torch.full_like(pool.host_offsets, -9)

    class _Event:
        def record(self):
            pass

        def synchronize(self):
            pass
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    pool.upload()
    assert pool.offsets.tolist() == [0, 3, 4, 9, 9, 9, 9]
    assert torch.equal(pool.geom[:9], pool.host_geom[:9]) and not bool(pool.geom[9:].any())
    assert pool.bytes_uploaded == 9 * (8 + 8 + 5) * 4 + 7 * 8
    pool.reset()
    assert pool.rows == 0 and pool.frames == 0 and pool.add(("vp", 1), *frames[1]) == 0


def test_record_pool_capacity_errors_name_the_capacity():
    rs = np.random.RandomState(2)
    pool = _pool(capacity_rows=6, capacity_frames=2)
    pool.add(0, *_frame(rs, 4))
    with pytest.raises(ValueError, match="capacity_rows = 6"):
        pool.add(1, *_frame(rs, 3))
    assert pool.frames == 1 and pool.rows == 4                          # nothing half-added
    pool.add(1, *_frame(rs, 2))
    with pytest.raises(ValueError, match="capacity_frames = 2"):
        pool.add(2, *_frame(rs, 1))
    with pytest.raises(ValueError, match="positive"):
        _pool(capacity_rows=0)
    nopr = _pool(probs=False)
    assert nopr.host_probs is None and nopr.add(0, *_frame(rs, 2)[:2]) == 0
    with pytest.raises(ValueError, match="probs"):
        nopr.add(1, *_frame(rs, 2))


def test_make_record_pool_and_the_statement_against_the_frame_by_frame_readers():
    """synth.make_record_pool is deterministic and ragged; expanding it with the statement equals finishing every frame like a reader
    (frame_ref) and padding it like the reference's dataset (the ragged statement on the finished frames)."""
    from ragged_pool_ref import expand_ragged_ref
    from ytvln import synth
    from ytvln.batch import RecordPool
    bs, K, T, frames, boxes, F, C = 3, 7, 24, 6, 5, 16, 9
    for viewpoints in (0, 5):
        made = synth.make_record_pool(bs, K, T, frames, boxes, F=F, C=C, seed=11, viewpoints=viewpoints)
        again = synth.make_record_pool(bs, K, T, frames, boxes, F=F, C=C, seed=11, viewpoints=viewpoints)
        frames_list, options, tokens, instr_mask, view = made
        assert all(np.array_equal(x, y) for a, b in zip(frames_list, again[0]) for x, y in zip(a, b)) and options == again[1]
        assert all(x.dtype == np.float32 for fr in frames_list for x in fr) and frames_list[0][1].shape[1] == 8
        ns = [len(fr[0]) for fr in frames_list]
        assert min(ns) >= 1 and max(ns) <= boxes + 3 and any(n + 1 > boxes for n in ns) and any(n + 1 < boxes for n in ns)
        assert tokens.shape == (bs, K, T) and instr_mask.shape == (bs, K, T) and len(options) == bs and all(len(o) == K for o in options)
        if viewpoints:
            assert len(frames_list) == viewpoints and view.shape == (bs, K, frames, 2) and view.dtype == np.float64
            assert all(fr[1][:, 6:].any() for fr in frames_list)
        else:
            assert view is None and any(len(set(fr[1][:, 4])) > 1 for fr in frames_list)       # two records, two image sizes
        pool = RecordPool(sum(ns), len(frames_list), feature_dim=F, num_classes=C, device=None)
        for i, fr in enumerate(frames_list):
            pool.add(i, *fr)
        index = RecordPool.index(options, frames)
        assert bool((index == -1).any())
        offs = pool.host_offsets.numpy()[:pool.frames + 1]
        got = expand_records_ref(pool.host_features.numpy(), pool.host_geom.numpy(), pool.host_probs.numpy(), offs, index.numpy(), boxes, view)
        assert got[4] == 0
        if view is None:                   # frame by frame, then the ragged statement
            done = [frame_ref(*fr) for fr in frames_list]
            off2 = np.concatenate([[0], np.cumsum([len(d[0]) for d in done])]).astype(np.int64)
            want = expand_ragged_ref(*(np.concatenate([d[i] for d in done]) for i in range(3)), off2, index.numpy(), boxes)
            assert all(np.array_equal(a, b) for a, b in zip(got[:4], want[:4]))
        else:                              # per slot: the slot's own headings
            f, bx, pr, m, _ = (a.reshape(bs, K, frames, boxes, -1) if a is not None and np.ndim(a) else a for a in got)
            for i, k, pos in ((0, 0, 0), (1, 3, 1), (2, 6, 2)):
                wf, wl, wp = frame_ref(*frames_list[options[i][k][pos]], view=view[i, k, pos])
                n = min(len(wf), boxes)
                assert np.array_equal(f[i, k, pos, :n], wf[:n]) and np.array_equal(bx[i, k, pos, :n, :11], wl[:n]) and np.array_equal(pr[i, k, pos, :n], wp[:n])
                assert not f[i, k, pos, n:].any() and m[i, k, pos].reshape(-1).tolist() == [1] * n + [0] * (boxes - n)


def test_statement_counts_bad_slots_and_the_empty_frame():
    pf, pg, pp, offsets, index, view = grid_records(6, 6, 21)
    good = expand_records_ref(pf, pg, pp, offsets, index, 6, view)
    assert good[4] == 0
    idx = index.copy()
    idx[1, 2, 1], idx[2, 0, 0] = len(offsets) - 1, -5
    assert expand_records_ref(pf, pg, pp, offsets, idx, 6, view)[4] == 2
    empty = offsets.copy()
    p = int(index[0, 0, 0])
    empty[p + 1] = empty[p]                                             # frame p is empty now (and p + 1 longer)
    out = expand_records_ref(pf, pg, pp, empty, index, 6, view)
    assert out[4] == int((index == p).sum()) and not out[3].reshape(3, 7, 4, 6)[0, 0, 0].any()
    assert not global_rows_ref(pf, empty)[p].any() and np.array_equal(global_rows_ref(pf, offsets)[p], sequential_mean(pf[offsets[p]:offsets[p + 1]]))


def test_global_rows_and_expand_records_check_arguments_without_a_device():
    from ytvln.batch import expand_records, global_rows
    pf, pg, pp, offsets, index, view = (torch.from_numpy(a) for a in grid_records(6, 8, 5))
    P = offsets.numel() - 1
    glob = torch.zeros(P, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        global_rows(pf, offsets)
    with pytest.raises(RuntimeError, match="GPU"):
        global_rows(pf, offsets, out=glob)
    with pytest.raises(ValueError, match="pool_features"):
        global_rows(pf.double(), offsets)
    with pytest.raises(ValueError, match="offsets"):
        global_rows(pf, offsets.int())
    with pytest.raises(ValueError, match="offsets"):
        global_rows(pf, offsets[:0])
    with pytest.raises(ValueError, match="out"):
        global_rows(pf, offsets, out=glob[:-1])
    with pytest.raises(ValueError, match="contiguous"):
        global_rows(pf.t().contiguous().t(), offsets)

    with pytest.raises(RuntimeError, match="GPU"):
        expand_records(pf, pg, pp, glob, offsets, index, 6)
    with pytest.raises(RuntimeError, match="GPU"):
        expand_records(pf, pg, None, glob, offsets, index, 6, view=view)
    with pytest.raises(ValueError, match="pool_geom"):
        expand_records(pf, pg[:-1], pp, glob, offsets, index, 6)                # rows disagree
    with pytest.raises(ValueError, match="pool_geom"):
        expand_records(pf, pg[:, :6].contiguous(), pp, glob, offsets, index, 6)   # eight columns, no fewer
    with pytest.raises(ValueError, match="pool_probs"):
        expand_records(pf, pg, pp.double(), glob, offsets, index, 6)
    with pytest.raises(ValueError, match="pool_features"):
        expand_records(pf.double(), pg, pp, glob, offsets, index, 6)
    with pytest.raises(ValueError, match="pool_global"):
        expand_records(pf, pg, pp, glob[:-1], offsets, index, 6)
    with pytest.raises(ValueError, match="pool_global"):
        expand_records(pf, pg, pp, torch.zeros(P, 7), offsets, index, 6)
    with pytest.raises(ValueError, match="offsets"):
        expand_records(pf, pg, pp, glob, offsets.int(), index, 6)
    with pytest.raises(ValueError, match="index"):
        expand_records(pf, pg, pp, glob, offsets, index.reshape(-1), 6)
    with pytest.raises(ValueError, match="index"):
        expand_records(pf, pg, pp, glob, offsets, index.int(), 6)
    with pytest.raises(ValueError, match="boxes"):
        expand_records(pf, pg, pp, glob, offsets, index, 0)
    with pytest.raises(ValueError, match="view"):
        expand_records(pf, pg, pp, glob, offsets, index, 6, view=view.float())  # fp64: the headings are Python floats in the reference
    with pytest.raises(ValueError, match="view"):
        expand_records(pf, pg, pp, glob, offsets, index, 6, view=view[:, :, :, :1].contiguous())
    with pytest.raises(ValueError, match="contiguous"):
        expand_records(pf.t().contiguous().t(), pg, pp, glob, offsets, index, 6)
    bs, K, frames = index.shape
    out = [torch.empty(bs, K, frames * 6, 8), torch.empty(bs, K, frames * 6, 12), torch.empty(bs, K, frames * 6, 5),
           torch.empty(bs, K, frames * 6, dtype=torch.int64)]
    with pytest.raises(RuntimeError, match="GPU"):
        expand_records(pf, pg, pp, glob, offsets, index, 6, out=out)
    with pytest.raises(ValueError, match=r"out\[3\]"):
        expand_records(pf, pg, pp, glob, offsets, index, 6, out=out[:3] + [out[3].int()])
    with pytest.raises(ValueError, match=r"out\[0\]"):
        expand_records(pf, pg, pp, glob, offsets, index, 6, out=[out[0][:, :, :-1]] + out[1:])
    with pytest.raises(ValueError, match="go together"):
        expand_records(pf, pg, None, glob, offsets, index, 6, out=out)
    with pytest.raises(ValueError, match="bad"):
        expand_records(pf, pg, pp, glob, offsets, index, 6, bad=torch.zeros(2, dtype=torch.int64))


def test_c_entry_points_reject_bad_arguments_without_a_launch():
    from ytvln import _lib
    lib = _lib.load()
    one = 64                                                            # any non-null address: nothing is dereferenced on the host
    ok = dict(pf=one, off=one, frames_in_pool=2, rows=4, F=8, out=one, stream=None)

    def rc_global(**kw):
        a = dict(ok)
        a.update(kw)
        return lib.ytvln_pool_global_rows_f32(*a.values())
    assert rc_global(frames_in_pool=0) == 0                             # nothing to do: no launch either
    for kw, word in ((dict(off=None), b"null"), (dict(out=None), b"null"), (dict(pf=None), b"null"), (dict(rows=-1), b"negative"),
                     (dict(frames_in_pool=-1), b"negative"), (dict(F=-1), b"negative"), (dict(frames_in_pool=2 ** 62), b"overflow")):
        assert rc_global(**kw) != 0, kw
        assert word in lib.ytvln_last_error(), (kw, lib.ytvln_last_error())

    ok = dict(pf=one, pg=one, pp=one, glob=one, off=one, frames_in_pool=2, rows=4, idx=one, view=None, slots=8, frames=4, boxes=3, F=8, C=5,
              of=one, ob=one, op=one, om=one, bad=None, stream=None)

    def rc(**kw):
        a = dict(ok)
        a.update(kw)
        return lib.ytvln_expand_records_f32(*a.values())
    assert rc(slots=0) == 0
    for kw, word in ((dict(off=None), b"null"), (dict(idx=None), b"null"), (dict(of=None), b"null"), (dict(ob=None), b"null"),
                     (dict(om=None), b"null"), (dict(pf=None), b"null"), (dict(pg=None), b"null"), (dict(glob=None), b"null"),
                     (dict(rows=-1), b"negative"), (dict(frames_in_pool=-1), b"negative"), (dict(slots=-4), b"negative"), (dict(F=-1), b"negative"),
                     (dict(boxes=0), b"negative"), (dict(frames=0), b"frames"), (dict(slots=9), b"multiple"), (dict(pp=None), b"go together"),
                     (dict(op=None), b"go together"), (dict(C=0), b"C > 0"), (dict(slots=2 ** 62), b"overflow")):
        assert rc(**kw) != 0, kw
        assert word in lib.ytvln_last_error(), (kw, lib.ytvln_last_error())
