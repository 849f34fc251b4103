"""Generate tests/golden/g22_action_masking.npz by RUNNING the reference's `randomize_tokens` (utils/dataset/common.py:213-270) with
`args.mask_action_rate` > 0, once per dataset item, on the CPU.

TEST INFRASTRUCTURE ONLY; runs where the reference checkout exists (oracle/ref_import.py).  Only data is written.  Usage:

    python tools/gen_golden_action_masking.py

The reference draws inside the function: torch.rand_like / torch.randint_like (torch's global generator), then np.random.choice (numpy's
global generator).  Both are seeded per item, and the same seeds replayed outside give the identical draws, which are stored next to the
inputs and the outputs so that the HIP kernel and the numpy restatement (tests/action_masking_ref.py) can be checked bit for bit.  The
script re-runs the reference on the recorded state and aborts on any mismatch, and asserts that the situations the tests rely on occur.

  case   items  K x T    group  rate
  a      5      3 x 100  300    0.3    crosses a 256-token chunk; not a multiple of 64
  b      4      7 x 80   560    1.0    the pre-training size
  c      3      1 x 24   24     2.5    less than one wave; m > n: repeats are certain
  d      2      2 x 64   128    0.7    item 0: n = 10 -> m = 7 (0.7 * 10 = 7.000000000000001 in double; a rate rounded to fp32 gives 6); item 1: n = 0

Item 0 of every case has action ids planted at the group indices 0, 63, 64, 255, 256 and group - 1 that exist (wave, chunk and row
boundaries; the last one lies in the padding: mask == 0).  Per case `x` the file holds x_tokens, x_mask [items, K, T], x_p (fp32), x_rnd,
x_choice [items, cap] (the np.random.choice result, -1 past m), x_out, x_tgt, x_counts [items, 2] = (n, m) and x_rate (float64).
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_import  # noqa: E402

ref_import.install_stubs()
sys.path.insert(0, ref_import.REFERENCE_ROOT)
import utils.dataset.common as C  # noqa: E402

V, MASK_ID = 30522, 103
ACTIONS = (2187, 2830, 2157)
vocab = {str(i): i for i in range(V)}
del vocab[str(MASK_ID)]
vocab["[MASK]"] = MASK_ID
tokenizer = types.SimpleNamespace(vocab=vocab)

CASES = {"a": (5, 3, 100, 0.3), "b": (4, 7, 80, 1.0), "c": (3, 1, 24, 2.5), "d": (2, 2, 64, 0.7)}
EDGES = (0, 63, 64, 255, 256)


def make_item(rng, K, T, plan):
    """One item: K instructions of random words with random lengths (zero-padded like the loader's), no action word by accident, then the
    action ids of `plan` = {flat position: id}."""
    tokens = rng.integers(1000, V, size=(K, T))
    for bad in ACTIONS + (MASK_ID,):
        tokens[tokens == bad] = bad + 1
    lens = rng.integers(max(T // 4, 1), max(T - 2, 2), size=K)
    mask = (np.arange(T)[None, :] < lens[:, None]).astype(np.int64)
    tokens = tokens * mask
    tokens[:, 0] = 101
    flat = tokens.reshape(-1)
    for pos, a in plan.items():
        flat[pos] = a
    return tokens, mask


def plans(name, rng, items, group):
    """{flat position: action id} per item"""
    out = []
    for it in range(items):
        plan = {}
        if name == "d":
            if it == 0:       # n = 10: the four edges that exist and six more
                for k, pos in enumerate([0, 63, 64, group - 1, 5, 17, 30, 70, 90, 100]):
                    plan[pos] = ACTIONS[k % 3]
        elif name == "c":
            pos = {0: [0, 23, 3, 4, 9, 15], 1: [7], 2: [1, 2, 11, 12]}[it]
            plan = {q: ACTIONS[(k + it) % 3] for k, q in enumerate(pos)}
        elif name == "a" and it == 1:
            plan = {40: ACTIONS[1], 141: ACTIONS[0]}                                   # n = 2 -> m = int(0.6) = 0
        elif name == "a" and it == 2:
            plan = {int(q): ACTIONS[2] for q in rng.choice(group, 12, replace=False)}   # a single class, the LAST of the three
        else:
            count = int(rng.integers(group // 12, group // 6))
            for q in rng.choice(group, count, replace=False):
                plan[int(q)] = ACTIONS[int(rng.integers(3))]
            if it == 0:
                for k, q in enumerate(EDGES + (group - 1,)):
                    if q < group:
                        plan[q] = ACTIONS[k % 3]
        out.append(plan)
    return out


def run_reference(tokens, mask, rate, seed):
    torch.manual_seed(seed)
    np.random.seed(seed + 1000)
    out, tgt = C.randomize_tokens(torch.from_numpy(tokens).clone(), torch.from_numpy(mask), tokenizer, types.SimpleNamespace(mask_action_rate=rate))
    return out.numpy(), tgt.numpy()


def record_draws(tokens, rate, seed):
    """The same seeds, the same calls in the same order as common.py:228-229 and :248."""
    torch.manual_seed(seed)
    t = torch.from_numpy(tokens)
    p = torch.rand_like(t.float())
    rnd = torch.randint_like(t, len(tokenizer.vocab))
    n = int(sum(int((tokens == a).sum()) for a in ACTIONS))
    np.random.seed(seed + 1000)
    choice = np.random.choice(range(n), int(rate * n))
    return p.numpy(), rnd.numpy(), np.asarray(choice, dtype=np.int64), n


def main():
    store = {}
    seen = dict(repeat=False, drawn_high_p=False, m0=False, single_class=False, under_mask0=False)
    for ci, (name, (items, K, T, rate)) in enumerate(CASES.items()):
        rng = np.random.default_rng(2200 + ci)
        group = K * T
        rows = []
        for it, plan in enumerate(plans(name, rng, items, group)):
            tokens, mask = make_item(rng, K, T, plan)
            seed = 22000 + 100 * ci + it
            out, tgt = run_reference(tokens, mask, rate, seed)
            p, rnd, choice, n = record_draws(tokens, rate, seed)
            out2, tgt2 = run_reference(tokens, mask, rate, seed)
            if not (np.array_equal(out, out2) and np.array_equal(tgt, tgt2)):
                raise SystemExit(f"case {name} item {it}: the reference does not replay under the same seeds")
            m = len(choice)
            # the recorded draws must explain the reference's output: positions in enumeration order, hit counts
            flat = tokens.reshape(-1)
            pos = np.concatenate([np.flatnonzero(flat == a) for a in ACTIONS])
            hits = np.bincount(choice, minlength=max(n, 1))[:n] if m else np.zeros(n, np.int64)
            drawn = pos[hits > 0]
            o, g = out.reshape(-1), tgt.reshape(-1)
            if not (np.all(o[drawn] == MASK_ID) and np.all(g[pos[hits == 1]] == flat[pos[hits == 1]]) and np.all(g[pos[hits > 1]] == MASK_ID)):
                raise SystemExit(f"case {name} item {it}: recorded draws do not reproduce the reference's output")
            pm = p.reshape(-1) * mask.reshape(-1)
            rest = np.ones(group, bool)
            rest[drawn] = False
            if not np.array_equal(g[rest] != -1, pm[rest] >= np.float32(0.85)):
                raise SystemExit(f"case {name} item {it}: recorded p does not reproduce the reference's targets")
            seen["repeat"] |= bool((hits > 1).any())
            seen["drawn_high_p"] |= bool((pm[drawn] >= np.float32(0.97)).any())
            seen["m0"] |= m == 0 < n
            seen["single_class"] |= n > 0 and sum(int((flat == a).any()) for a in ACTIONS) == 1
            seen["under_mask0"] |= bool((mask.reshape(-1)[drawn] == 0).any())
            rows.append((tokens, mask, p, rnd, choice, out, tgt, (n, m)))
        if name == "d":
            assert rows[0][7] == (10, 7) and rows[1][7] == (0, 0), [r[7] for r in rows]
        cap = max(max(len(r[4]) for r in rows), 1)
        ch = np.full((items, cap), -1, np.int64)
        for it, r in enumerate(rows):
            ch[it, :len(r[4])] = r[4]
        for key, idx in (("tokens", 0), ("mask", 1), ("p", 2), ("rnd", 3), ("out", 5), ("tgt", 6)):
            store[f"{name}_{key}"] = np.stack([r[idx] for r in rows])
        store[f"{name}_choice"] = ch
        store[f"{name}_counts"] = np.asarray([r[7] for r in rows], dtype=np.int64)
        store[f"{name}_rate"] = np.float64(rate)
        print(f"case {name}: (n, m) per item = {[r[7] for r in rows]}")
    assert all(seen.values()), seen
    path = os.path.join(ROOT, "tests", "golden", "g22_action_masking.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes;", seen)


if __name__ == "__main__":
    main()
