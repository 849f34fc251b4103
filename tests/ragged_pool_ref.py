"""Numpy statement of what ytvln_expand_ragged_f32 computes (include/ytvln.h), shared by test_ragged_pool_cpu.py and test_ragged_pool_gpu.py.

Per slot s = (item, option, position f): zeros; copy the first min(n, boxes) rows of pool frame p = index[s]; column 11 of the boxes = f;
mask 1 on the copied rows.  n = 0 for a padding frame (p = -1) and for a BAD slot: p >= pool_frames, p < -1, or offsets[p], offsets[p+1]
out of order or outside [0, pool_rows]; bad slots are counted."""
import numpy as np


def expand_ragged_ref(pool_features, pool_loc, pool_probs, offsets, index, boxes):
    """numpy in, numpy out: (features [bs, K, frames*boxes, F], boxes [.., 12], probs [.., C] or None, masks [..] int64, bad count)."""
    pool_rows, F = pool_features.shape
    L = pool_loc.shape[1]
    pool_frames = len(offsets) - 1
    bs, K, frames = index.shape
    slots = bs * K * frames
    f = np.zeros((slots, boxes, F), np.float32)
    bx = np.zeros((slots, boxes, 12), np.float32)
    pr = np.zeros((slots, boxes, pool_probs.shape[1]), np.float32) if pool_probs is not None else None
    m = np.zeros((slots, boxes), np.int64)
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
        if not 0 <= a <= b <= pool_rows:
            bad += 1
            continue
        n = min(b - a, boxes)
        f[s, :n] = pool_features[a:a + n]
        bx[s, :n, :L] = pool_loc[a:a + n]
        if pr is not None:
            pr[s, :n] = pool_probs[a:a + n]
        m[s, :n] = 1
    R = frames * boxes
    return (f.reshape(bs, K, R, F), bx.reshape(bs, K, R, 12), pr.reshape(bs, K, R, -1) if pr is not None else None, m.reshape(bs, K, R), bad)


def grid_pool(boxes, F, C, L=11, seed=5, P=23, bs=3, K=7, frames=4):
    """The shape grid of the GPU tests: P frames with n cycling through {1, 2, boxes-1, boxes, boxes+1, boxes+3} and one n = 0; options built
    like test_expand_options_matches_host_expansion (path lengths 2-4, so padding frames occur).  Returns numpy (pf, pl, pp, offsets, index)."""
    rs = np.random.RandomState(seed)
    ns = [(1, 2, boxes - 1, boxes, boxes + 1, boxes + 3)[i % 6] for i in range(P)]
    ns[7] = 0
    offsets = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    rows = int(offsets[-1])
    pf = np.maximum(rs.standard_normal((rows, F)), 0).astype(np.float32)
    pl = rs.uniform(0, 1, (rows, L)).astype(np.float32)
    pp = rs.uniform(0, 1, (rows, C)).astype(np.float32)
    index = np.full((bs, K, frames), -1, np.int64)
    for b in range(bs):
        Lp = 2 + b % 3
        path = np.array(((2, 4), (0, 3, 5), (1, 8, 10, 9))[b % 3]) + 6 * (b // 3)      # between them every kind of n
        index[b, 0, :Lp] = index[b, 1, :Lp] = index[b, 2, :Lp] = path
        index[b, 3, :Lp] = path[rs.permutation(Lp)]
        index[b, 4, :Lp] = path[rs.permutation(Lp)]
        for k in (5, 6):
            alt = path.copy()
            alt[rs.randint(0, Lp)] = rs.randint(0, P)
            index[b, k, :Lp] = alt
    index[0, 1, 0] = 7                       # the empty frame is shown too
    return pf, pl, pp, offsets, index
