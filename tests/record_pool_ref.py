"""Numpy statement of what ytvln_pool_global_rows_f32 and ytvln_expand_records_f32 compute (include/ytvln.h), shared by
test_record_pool_cpu.py and test_record_pool_gpu.py.  Written out as loops: the order of the fp32 additions is part of the contract.

A frame of n_src raw rows becomes n_src + 1 reader rows: the global region (sequential fp32 mean, whole-image box, 1 / C) and the rows
with their boxes normalised in fp32; the six orientation columns are 1 (photo readers) or the fp64 sine / cosine of the fp32 angle,
rounded once (panoramas).  A slot keeps the first min(n_src + 1, boxes) of them; an empty frame is a BAD slot."""
import numpy as np

from ragged_pool_ref import grid_pool


def sequential_mean(x):
    """[n, F] fp32 -> [F] fp32: (((0 + x[0]) + x[1]) + ... + x[n-1]) / fp32(n), every operation in fp32, rows in order."""
    acc = np.zeros(x.shape[1], np.float32)
    for r in range(x.shape[0]):
        acc = acc + x[r]
    assert acc.dtype == np.float32
    return acc / np.float32(x.shape[0])


def global_rows_ref(pool_features, offsets):
    pool_rows, F = pool_features.shape
    out = np.zeros((len(offsets) - 1, F), np.float32)
    for p in range(len(offsets) - 1):
        a, b = int(offsets[p]), int(offsets[p + 1])
        if 0 <= a < b <= pool_rows:
            out[p] = sequential_mean(pool_features[a:b])
    return out


def _trig(angle32):
    assert angle32.dtype == np.float32
    a = angle32.astype(np.float64)
    return np.sin(a).astype(np.float32), np.cos(a).astype(np.float32)


def locations_ref(geom, view=None):
    """[n, 8] fp32 raw geometry -> [n, 11] fp32 locations; view = (heading, next heading) or None."""
    assert geom.dtype == np.float32
    x1, y1, x2, y2, w, h, fh, fe = (geom[:, c] for c in range(8))
    loc = np.ones((len(geom), 11), np.float32)
    loc[:, 0], loc[:, 1], loc[:, 2], loc[:, 3] = x1 / w, y1 / h, x2 / w, y2 / h
    loc[:, 4] = ((x2 - x1) * (y2 - y1)) / (w * h)
    if view is not None:
        loc[:, 5], loc[:, 6] = _trig(fh - np.float32(view[0]))
        loc[:, 7], loc[:, 8] = _trig(fe)
        loc[:, 9], loc[:, 10] = _trig(fh - np.float32(view[1]))
    return loc


def global_location_ref(view=None):
    g = np.array([0, 0, 1, 1, 1, 0, 1, 0, 1, 0, 1], np.float32)
    if view is not None:
        for c, turn in ((5, view[0]), (9, view[1])):
            g[c], g[c + 1] = np.float32(np.sin(-np.float64(turn))), np.float32(np.cos(-np.float64(turn)))
    return g


def frame_ref(features, geom, probs, view=None):
    """What the reference's reader returns for these raw rows, after `.float()`: (features [n+1, F], locations [n+1, 11], probs [n+1, C])."""
    C = probs.shape[1]
    return (np.concatenate([sequential_mean(features)[None], features]), np.concatenate([global_location_ref(view)[None], locations_ref(geom, view)]),
            np.concatenate([np.full((1, C), np.float32(1.0 / C), np.float32), probs]))


def expand_records_ref(pool_features, pool_geom, pool_probs, offsets, index, boxes, view=None):
    """numpy in, numpy out: (features [bs, K, frames*boxes, F], boxes [.., 12], probs [.., C] or None, masks [..] int64, bad count)."""
    pool_rows, F = pool_features.shape
    pool_frames = len(offsets) - 1
    bs, K, frames = index.shape
    slots = bs * K * frames
    C = pool_probs.shape[1] if pool_probs is not None else 0
    f = np.zeros((slots, boxes, F), np.float32)
    bx = np.zeros((slots, boxes, 12), np.float32)
    pr = np.zeros((slots, boxes, C), np.float32) if pool_probs is not None else None
    m = np.zeros((slots, boxes), np.int64)
    turns = view.reshape(slots, 2) if view is not None else None
    bad = 0
    for s, p in enumerate(index.reshape(-1)):
        p = int(p)
        bx[s, :, 11] = s % frames
        if p == -1:
            continue
        if p < -1 or p >= pool_frames:
            bad += 1
            continue
        a, b = int(offsets[p]), int(offsets[p + 1])
        if not 0 <= a < b <= pool_rows:
            bad += 1
            continue
        n = min(b - a + 1, boxes)
        turn = turns[s] if turns is not None else None
        f[s, 0] = sequential_mean(pool_features[a:b])
        bx[s, 0, :11] = global_location_ref(turn)
        f[s, 1:n] = pool_features[a:a + n - 1]
        bx[s, 1:n, :11] = locations_ref(pool_geom[a:a + n - 1], turn)
        if pr is not None:
            pr[s, 0] = np.float32(1.0 / C)
            pr[s, 1:n] = pool_probs[a:a + n - 1]
        m[s, :n] = 1
    R = frames * boxes
    return (f.reshape(bs, K, R, F), bx.reshape(bs, K, R, 12), pr.reshape(bs, K, R, -1) if pr is not None else None, m.reshape(bs, K, R), bad)


def mixed_magnitudes(rs, shape):
    """fp32 values whose magnitudes span six decades, both signs: a sum over them depends on the order of the additions."""
    return (rs.standard_normal(shape) * 10.0 ** rs.uniform(-3, 3, shape)).astype(np.float32)


def grid_records(boxes, F, C, seed=5, P=23):
    """The shape grid of the GPU tests: P frames with n_src cycling through {1, 2, boxes-2, boxes-1, boxes, boxes+3}; every third frame of
    two or more rows is two records with different image sizes; the option set of ragged_pool_ref.grid_pool (path lengths 2-4, so padding
    frames occur); one (heading, next heading) per slot.  Returns numpy (pf, pg, pp, offsets, index, view)."""
    rs = np.random.RandomState(seed)
    ns = [(1, 2, boxes - 2, boxes - 1, boxes, boxes + 3)[i % 6] for i in range(P)]
    offsets = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    rows = int(offsets[-1])
    pf = np.maximum(rs.standard_normal((rows, F)), 0).astype(np.float32)
    pg = np.zeros((rows, 8), np.float32)
    for i, n in enumerate(ns):
        a = int(offsets[i])
        cut = n // 2 if (i % 3 == 2 and n >= 2) else n
        for lo, hi in ((a, a + cut), (a + cut, a + n)):
            w, h = rs.randint(300, 900, size=2)
            xy = np.sort(rs.uniform(0, 1, (hi - lo, 2, 2)), axis=-1)
            pg[lo:hi, 0], pg[lo:hi, 2], pg[lo:hi, 1], pg[lo:hi, 3] = xy[:, 0, 0] * w, xy[:, 0, 1] * w, xy[:, 1, 0] * h, xy[:, 1, 1] * h
            pg[lo:hi, 4], pg[lo:hi, 5] = w, h
    pg[:, 6:8] = rs.uniform(-3.1, 3.1, (rows, 2))
    pp = rs.uniform(0, 1, (rows, C)).astype(np.float32)
    index = grid_pool(boxes, 1, 1, P=P)[4]
    view = rs.uniform(-np.pi, np.pi, index.shape + (2,))
    return pf, pg, pp, offsets, index, view
