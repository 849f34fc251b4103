"""numpy restatement of the reference's `randomize_tokens` with `mask_action_rate` > 0 (utils/dataset/common.py:213-270).  TEST
INFRASTRUCTURE: the yardstick of tests/test_action_masking_*.py, itself pinned to the reference's own outputs by
tests/golden/g22_action_masking.npz (tools/gen_golden_action_masking.py runs the reference).

What the reference does per dataset item (tokens [K, T], all K instructions together):
  common.py:225-229   targets = -1;  p = U[0,1) * mask;  random_tokens = randint(vocab)
  common.py:235-244   the positions of 2187, then of 2830, then of 2157, each in row-major order (torch.where per id, concatenated): n
  common.py:248       mask_index = np.random.choice(range(n), int(rate * n))        with replacement; a product of Python floats (doubles)
  common.py:250-253   for every drawn ordinal IN ORDER: targets[pos] = tokens[pos]; tokens[pos] = [MASK]; p[pos] = 0.85 * 0.9
                      -- the read of tokens[pos] sees the write of an earlier draw: a position drawn twice ends with target = [MASK]
  common.py:255-268   thresholds 0.85 / 0.97 / 0.985 on p; a drawn position has p = 0.765 and is not touched again
The action step never looks at `mask`.
"""
import numpy as np

ACTION_TOKEN_IDS = (2187, 2830, 2157)
MASK_TOKEN_ID = 103
# the thresholds as torch compares an fp32 tensor with a Python double: the scalar is rounded to fp32 first
T_MASK, T_RANDOM, T_KEEP = np.float32(0.85), np.float32(0.85 + 0.15 * 0.8), np.float32(0.85 + 0.15 * 0.9)


def draw_count(rate, n):
    """int(mask_action_rate * len(action_positions)) of common.py:248: a double product truncated toward zero."""
    return int(float(rate) * n)


def action_positions(tokens_flat, action_tokens=ACTION_TOKEN_IDS):
    """flat positions in the reference's enumeration order (common.py:238-244)"""
    return np.concatenate([np.flatnonzero(tokens_flat == a) for a in action_tokens])


def randomize_tokens_action(tokens, mask, p, random_tokens, choice, rate, items, action_tokens=ACTION_TOKEN_IDS,
                            mask_token_id=MASK_TOKEN_ID, repeat_target="reference"):
    """tokens / mask / p / random_tokens: arrays of items * group elements (any shape); choice: [items, cap] drawn ordinals, of which the
    first min(m, cap) of a row are used and values outside [0, n) are skipped.  Returns (out, targets, counts [items, 2] = (n, m))."""
    assert repeat_target in ("reference", "token")
    shape = np.shape(tokens)
    tok = np.asarray(tokens, dtype=np.int64).reshape(items, -1)
    msk = np.asarray(mask).reshape(items, -1).astype(np.float32)
    pp = np.asarray(p, dtype=np.float32).reshape(items, -1) * msk
    rnd = np.asarray(random_tokens, dtype=np.int64).reshape(items, -1)
    choice = np.zeros((items, 0), np.int64) if choice is None else np.asarray(choice, dtype=np.int64).reshape(items, -1)
    out, tgt = tok.copy(), np.full_like(tok, -1)
    counts = np.zeros((items, 2), np.int64)
    for it in range(items):
        pos = action_positions(tok[it], action_tokens)
        n, m = len(pos), draw_count(rate, len(pos))
        counts[it] = (n, m)
        drawn = [int(c) for c in choice[it, :min(m, choice.shape[1])] if 0 <= c < n]
        t, g, q = out[it], tgt[it], pp[it].copy()
        for c in drawn:                                   # common.py:250-253, draw by draw
            g[pos[c]] = t[pos[c]]
            t[pos[c]] = mask_token_id
            q[pos[c]] = np.float32(0.85 * 0.9)
        if repeat_target == "token":
            hit = pos[np.asarray(drawn, dtype=np.int64)]
            g[hit] = tok[it][hit]
        sel = q >= T_MASK                                 # common.py:255-268
        g[sel] = t[sel]
        t[sel] = mask_token_id
        sel = q >= T_RANDOM
        t[sel] = rnd[it][sel]
        sel = q >= T_KEEP
        t[sel] = g[sel]
    return out.reshape(shape), tgt.reshape(shape), counts
