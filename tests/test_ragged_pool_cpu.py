"""CPU: host logic of the ragged frame pool (ytvln.batch.RaggedPool, expand_ragged's argument checks, synth.make_ragged_pool) and the
numpy reference of the kernel (tests/ragged_pool_ref.py) against a frame-by-frame host padding loop."""
import numpy as np
import pytest
import torch

from ragged_pool_ref import expand_ragged_ref, grid_pool


def _frame(rs, n, F=8, C=5, dtype=np.float64):
    return rs.standard_normal((n, F)).astype(np.float32), rs.uniform(0, 1, (n, 11)).astype(dtype), rs.uniform(0, 1, (n, C)).astype(dtype)


def _pool(**kw):
    from ytvln.batch import RaggedPool
    args = dict(capacity_rows=20, capacity_frames=6, feature_dim=8, loc_dim=11, num_classes=5, device=None)
    args.update(kw)
    pool = RaggedPool(**args)
    if pool.device is not None:            # a GPU happens to be present: these tests are about the host side only
        pool.device = None
    return pool


def test_ids_offsets_dedup_and_conversion():
    rs = np.random.RandomState(0)
    pool = _pool()
    frames = [_frame(rs, n) for n in (3, 1, 5)]
    ids = [pool.add(("k", i), *fr) for i, fr in enumerate(frames)]
    assert ids == [0, 1, 2] and pool.frames == 3 and pool.rows == 9
    assert pool.host_offsets[:4].tolist() == [0, 3, 4, 9]
    for (f, loc, pr), a, b in zip(frames, (0, 3, 4), (3, 4, 9)):
        assert torch.equal(pool.host_features[a:b], torch.from_numpy(f))
        assert torch.equal(pool.host_locations[a:b], torch.from_numpy(loc).float())        # fp64 -> fp32 as `.float()` does
        assert torch.equal(pool.host_probs[a:b], torch.from_numpy(pr).float())
    assert pool.host_locations.dtype == torch.float32 and not torch.equal(pool.host_locations[0:3].double(), torch.from_numpy(frames[0][1]))
    # a key seen before: its id, and nothing is copied even when other arrays come with it
    before = [t.clone() for t in (pool.host_features, pool.host_locations, pool.host_probs, pool.host_offsets)]
    assert pool.add(("k", 1), *_frame(rs, 4)) == 1
    assert pool.frames == 3 and pool.rows == 9
    for t, b in zip((pool.host_features, pool.host_locations, pool.host_probs, pool.host_offsets), before):
        assert torch.equal(t, b)
    # fp32 input is taken as it is
    f, loc, pr = _frame(rs, 2, dtype=np.float32)
    assert pool.add("fp32", f, loc, pr) == 3
    assert torch.equal(pool.host_locations[9:11], torch.from_numpy(loc)) and torch.equal(pool.host_probs[9:11], torch.from_numpy(pr))
    # reset: ids start again, keys are forgotten
    pool.reset()
    assert pool.frames == 0 and pool.rows == 0
    assert pool.add(("k", 1), *frames[1]) == 0


def test_max_rows_truncates_like_the_reference():
    rs = np.random.RandomState(1)
    pool = _pool()
    f, loc, pr = _frame(rs, 7)
    assert pool.add("a", f, loc, pr, max_rows=4) == 0
    assert pool.rows == 4 and pool.host_offsets[1] == 4                 # num_boxes = min(len, max_num_boxes): the FIRST rows
    assert torch.equal(pool.host_features[:4], torch.from_numpy(f[:4])) and torch.equal(pool.host_probs[:4], torch.from_numpy(pr[:4]).float())
    assert pool.add("b", *_frame(rs, 2), max_rows=4) == 1 and pool.rows == 6


def test_capacity_errors_name_the_capacity():
    rs = np.random.RandomState(2)
    pool = _pool(capacity_rows=6, capacity_frames=2)
    pool.add(0, *_frame(rs, 4))
    with pytest.raises(ValueError, match="capacity_rows = 6"):
        pool.add(1, *_frame(rs, 3))
    assert pool.frames == 1 and pool.rows == 4                          # nothing half-added
    pool.add(1, *_frame(rs, 2))
    with pytest.raises(ValueError, match="capacity_frames = 2"):
        pool.add(2, *_frame(rs, 0))
    with pytest.raises(ValueError):
        pool.add(3, np.zeros((2, 8), np.int32), np.zeros((2, 11)), np.zeros((2, 5)))


def test_offsets_tail_repeats_the_last_value_and_device_calls_need_the_gpu():
    rs = np.random.RandomState(3)
    pool = _pool()
    pool.add(0, *_frame(rs, 2))
    pool.add(1, *_frame(rs, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        pool.upload()
    with pytest.raises(RuntimeError, match="GPU"):
        pool.expand(torch.zeros(1, 1, 1, dtype=torch.int64), 4)
    pool.host_offsets[pool.frames + 1:] = pool.rows                     # what upload() does before it copies
    assert pool.host_offsets.tolist() == [0, 2, 5, 5, 5, 5, 5]


def test_upload_fills_the_offsets_tail(monkeypatch):
    """upload() itself, with the device copies replaced by host ones: the tail of offsets repeats the last value and bytes_uploaded counts
    the used rows only."""
    rs = np.random.RandomState(4)
    pool = _pool()
    pool.add(0, *_frame(rs, 2))
    pool.add(1, *_frame(rs, 3))
    pool.device = torch.device("cpu")
    pool.features, pool.locations, pool.probs = (torch.zeros_like(t) for t in (pool.host_features, pool.host_locations, pool.host_probs))
    pool.offsets = torch.full_like(pool.host_offsets, -9)

    class _Event:
        def record(self):
            pass

        def synchronize(self):
            pass
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    pool.upload()
    assert pool.offsets.tolist() == [0, 2, 5, 5, 5, 5, 5]
    assert torch.equal(pool.features[:5], pool.host_features[:5]) and not bool(pool.features[5:].any())
    assert pool.bytes_uploaded == 5 * (8 + 11 + 5) * 4 + 7 * 8
    pool.reset()
    assert pool.rows == 0


def test_index_truncates_and_pads():
    from ytvln.batch import RaggedPool
    idx = RaggedPool.index([[[0, 1, 2, 3, 4], [2]], [[], [5, 6, 7]]], 3)
    assert idx.dtype == torch.int64 and idx.shape == (2, 2, 3)
    assert idx.tolist() == [[[0, 1, 2], [2, -1, -1]], [[-1, -1, -1], [5, 6, 7]]]
    with pytest.raises(ValueError):
        RaggedPool.index([[[0]], [[1], [2]]], 3)


def _host_padding_loop(frames_list, options, frames, boxes, F, C):
    """The reference's dataset code, frame by frame (utils/dataset/all_dataset.py:294-345), for nested id lists."""
    bs, K = len(options), len(options[0])
    f = np.zeros((bs, K, frames, boxes, F))
    bx = np.zeros((bs, K, frames, boxes, 12))
    pr = np.zeros((bs, K, frames, boxes, C))
    m = np.zeros((bs, K, frames, boxes), np.int64)
    for i in range(bs):
        for k in range(K):
            for pos in range(frames):
                bx[i, k, pos, :, 11] = pos
                if pos < len(options[i][k]):
                    feat, loc, probs = frames_list[options[i][k][pos]]
                    n = min(len(loc), boxes)
                    f[i, k, pos, :n] = feat[:n]
                    bx[i, k, pos, :n, :11] = loc[:n, :11]
                    pr[i, k, pos, :n] = probs[:n]
                    m[i, k, pos, :n] = 1
    R = frames * boxes
    t = lambda a: torch.from_numpy(a.reshape(bs, K, R, -1)).float()          # noqa: E731  (fp64 padded on the host, then `.float()`)
    return t(f), t(bx), t(pr), torch.from_numpy(m.reshape(bs, K, R))


def test_reference_equals_the_host_padding_loop_and_make_ragged_pool_is_ragged():
    from ytvln import synth
    from ytvln.batch import RaggedPool
    bs, K, T, frames, boxes, F, C = 3, 7, 24, 6, 5, 16, 9
    made = synth.make_ragged_pool(bs, K, T, frames, boxes, F=F, C=C, seed=11)
    again = synth.make_ragged_pool(bs, K, T, frames, boxes, F=F, C=C, seed=11)
    other = synth.make_ragged_pool(bs, K, T, frames, boxes, F=F, C=C, seed=12)
    frames_list, options, tokens, instr_mask = made
    assert all(np.array_equal(x, y) for a, b in zip(frames_list, again[0]) for x, y in zip(a, b)) and options == again[1]
    assert np.array_equal(tokens, again[2]) and not all(len(a[1]) == len(b[1]) for a, b in zip(frames_list, other[0]))
    ns = [len(fr[1]) for fr in frames_list]
    assert min(ns) >= 1 and max(ns) <= boxes + 3 and any(n > boxes for n in ns) and any(n < boxes for n in ns)
    assert frames_list[0][0].dtype == np.float32 and frames_list[0][1].dtype == np.float64 and frames_list[0][2].dtype == np.float64
    assert frames_list[0][1].shape[1] == 11 and tokens.shape == (bs, K, T) and instr_mask.shape == (bs, K, T)
    assert len(options) == bs and all(len(o) == K for o in options)
    assert all(options[i][1] == options[i][0] == options[i][2] for i in range(bs))          # caption negatives share the frames
    assert all(sorted(options[i][3]) == sorted(options[i][0]) for i in range(bs))           # frame permutations

    pool = RaggedPool(sum(min(n, boxes) for n in ns), len(frames_list), feature_dim=F, num_classes=C, device=None)
    ids = [pool.add(i, *fr, max_rows=boxes) for i, fr in enumerate(frames_list)]
    assert ids == list(range(len(frames_list)))
    index = RaggedPool.index(options, frames)
    assert bool((index == -1).any())
    offs = pool.host_offsets.numpy()
    rf, rb, rp, rm, bad = expand_ragged_ref(pool.host_features.numpy(), pool.host_locations.numpy(), pool.host_probs.numpy(), offs, index.numpy(), boxes)
    hf, hb, hp, hm = _host_padding_loop(frames_list, options, frames, boxes, F, C)
    assert bad == 0
    assert torch.equal(torch.from_numpy(rf), hf) and torch.equal(torch.from_numpy(rb), hb)
    assert torch.equal(torch.from_numpy(rp), hp) and torch.equal(torch.from_numpy(rm), hm)
    # the same without max_rows: the cut then happens in the expansion (n = min(rows of the frame, boxes))
    full = RaggedPool(sum(ns), len(frames_list), feature_dim=F, num_classes=C, device=None)
    for i, fr in enumerate(frames_list):
        full.add(i, *fr)
    out = expand_ragged_ref(full.host_features.numpy(), full.host_locations.numpy(), full.host_probs.numpy(), full.host_offsets.numpy(), index.numpy(), boxes)
    assert all(np.array_equal(a, b) for a, b in zip(out[:4], (rf, rb, rp, rm)))


def test_reference_equals_the_expand_options_host_expansion_when_every_frame_is_full():
    """n == boxes everywhere: the host expansion of test_expand_options_matches_host_expansion (pool_masks all ones), except column 11
    of padding frames, where the ragged form writes the position like the reference and expand_options writes 0."""
    g = torch.Generator().manual_seed(5)
    P, boxes, F, C, bs, K, frames = 23, 6, 64, 21, 3, 7, 4
    pf = torch.relu(torch.randn(P, boxes, F, generator=g))
    pb = torch.rand(P, boxes, 12, generator=g)
    pp = torch.softmax(torch.randn(P, boxes, C, generator=g), -1)
    index = torch.from_numpy(grid_pool(boxes, F, C)[4])
    safe, valid = index.clamp(min=0), index >= 0
    ef = (pf[safe] * valid[..., None, None]).reshape(bs, K, frames * boxes, F)
    eb = pb[safe] * valid[..., None, None]
    eb[..., 11] = torch.arange(frames).view(1, 1, frames, 1) * valid[..., None]
    ep = (pp[safe] * valid[..., None, None]).reshape(bs, K, frames * boxes, C)
    em = (torch.ones(P, boxes, dtype=torch.int64)[safe] * valid[..., None]).reshape(bs, K, frames * boxes)
    offsets = np.arange(P + 1, dtype=np.int64) * boxes
    rf, rb, rp, rm, bad = expand_ragged_ref(pf.reshape(-1, F).numpy(), pb[..., :11].reshape(-1, 11).numpy().copy(), pp.reshape(-1, C).numpy(),
                                            offsets, index.numpy(), boxes)
    assert bad == 0 and torch.equal(torch.from_numpy(rf), ef) and torch.equal(torch.from_numpy(rp), ep) and torch.equal(torch.from_numpy(rm), em)
    rb = torch.from_numpy(rb).view(bs, K, frames, boxes, 12)
    assert torch.equal(rb[..., :11], eb[..., :11])
    assert torch.equal(rb[..., 11][valid], eb[..., 11][valid])
    pad = ~valid
    assert bool(pad.any()) and torch.equal(rb[..., 11][pad], torch.arange(frames).view(1, 1, frames, 1).expand(bs, K, frames, boxes)[pad].float())


def test_reference_counts_bad_slots():
    pf, pl, pp, offsets, index = grid_pool(6, 6, 21)
    good = expand_ragged_ref(pf, pl, pp, offsets, index, 6)
    idx = index.copy()
    idx[1, 2, 1], idx[2, 0, 0] = len(offsets) - 1, -5
    out = expand_ragged_ref(pf, pl, pp, offsets, idx, 6)
    assert good[4] == 0 and out[4] == 2
    assert not out[3].reshape(3, 7, 4, 6)[1, 2, 1].any() and not out[0].reshape(3, 7, 4, 6, -1)[2, 0, 0].any()
    broken = offsets.copy()
    broken[4] = broken[3] - 1                                         # out of order: frames 3 and 4 both see a bad pair or a shifted one
    assert expand_ragged_ref(pf, pl, pp, broken, index, 6)[4] >= 1


def test_expand_ragged_checks_arguments_without_a_device():
    from ytvln.batch import expand_ragged
    pf, pl, pp, offsets, index = (torch.from_numpy(a) for a in grid_pool(6, 8, 5))
    with pytest.raises(RuntimeError, match="GPU"):
        expand_ragged(pf, pl, pp, offsets, index, 6)
    with pytest.raises(RuntimeError, match="GPU"):
        expand_ragged(pf, pl, None, offsets, index, 6)
    with pytest.raises(ValueError, match="pool_locations"):
        expand_ragged(pf, pl[:-1], pp, offsets, index, 6)                       # rows disagree
    with pytest.raises(ValueError, match="pool_probs"):
        expand_ragged(pf, pl, pp.double(), offsets, index, 6)
    with pytest.raises(ValueError, match="pool_features"):
        expand_ragged(pf.double(), pl, pp, offsets, index, 6)
    with pytest.raises(ValueError, match="offsets"):
        expand_ragged(pf, pl, pp, offsets.int(), index, 6)
    with pytest.raises(ValueError, match="index"):
        expand_ragged(pf, pl, pp, offsets, index.reshape(-1), 6)
    with pytest.raises(ValueError, match="index"):
        expand_ragged(pf, pl, pp, offsets, index.int(), 6)
    with pytest.raises(ValueError, match="boxes"):
        expand_ragged(pf, pl, pp, offsets, index, 0)
    with pytest.raises(ValueError, match="11"):
        expand_ragged(pf, torch.zeros(pf.shape[0], 12), pp, offsets, index, 6)
    with pytest.raises(ValueError, match="contiguous"):
        expand_ragged(pf.t().contiguous().t(), pl, pp, offsets, index, 6)
    bs, K, frames = index.shape
    out = [torch.empty(bs, K, frames * 6, 8), torch.empty(bs, K, frames * 6, 12), torch.empty(bs, K, frames * 6, 5),
           torch.empty(bs, K, frames * 6, dtype=torch.int64)]
    with pytest.raises(RuntimeError, match="GPU"):
        expand_ragged(pf, pl, pp, offsets, index, 6, out=out)
    with pytest.raises(ValueError, match=r"out\[3\]"):
        expand_ragged(pf, pl, pp, offsets, index, 6, out=out[:3] + [out[3].int()])
    with pytest.raises(ValueError, match=r"out\[0\]"):
        expand_ragged(pf, pl, pp, offsets, index, 6, out=[out[0][:, :, :-1]] + out[1:])
    with pytest.raises(ValueError, match="go together"):
        expand_ragged(pf, pl, None, offsets, index, 6, out=out)
    with pytest.raises(ValueError, match="bad"):
        expand_ragged(pf, pl, pp, offsets, index, 6, bad=torch.zeros(2, dtype=torch.int64))


def test_c_entry_point_rejects_bad_arguments_without_a_launch():
    from ytvln import _lib
    lib = _lib.load()
    one = 64                                                            # any non-null address: nothing is dereferenced on the host
    ok = dict(pf=one, pl=one, pp=one, off=one, frames_in_pool=2, rows=4, idx=one, slots=8, frames=4, boxes=3, F=8, L=11, C=5, of=one, ob=one,
              op=one, om=one, bad=None, stream=None)

    def rc(**kw):
        a = dict(ok)
        a.update(kw)
        return lib.ytvln_expand_ragged_f32(*a.values())
    assert rc(slots=0) == 0                                             # nothing to do: no launch either
    for kw, word in ((dict(off=None), b"null"), (dict(of=None), b"null"), (dict(om=None), b"null"), (dict(pf=None), b"null"),
                     (dict(rows=-1), b"negative"), (dict(frames_in_pool=-1), b"negative"), (dict(slots=-4), b"negative"), (dict(F=-1), b"negative"),
                     (dict(frames=0), b"frames"), (dict(slots=9), b"multiple"), (dict(L=12), b"L = 12"), (dict(pp=None), b"go together"),
                     (dict(op=None), b"go together")):
        assert rc(**kw) < 0, kw
        assert word in lib.ytvln_last_error(), (kw, lib.ytvln_last_error())
