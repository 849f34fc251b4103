"""GPU: action-aware token masking on the device (`ytvln.batch.randomize_tokens(..., mask_action_rate=r)`, csrc/batch.hip
randomize_tokens_action_kernel) against the golden made by running the reference (tests/golden/g22_action_masking.npz) and the numpy
restatement (tests/action_masking_ref.py)."""
import numpy as np
import pytest
import torch

import action_masking_ref as R
from helpers import gold

pytestmark = pytest.mark.gpu

CASES = {"a": (5, 300), "b": (4, 560), "c": (3, 24), "d": (2, 128)}
V = 30522


@pytest.fixture()
def stream_state():
    """the tests below seed / restore the library's mask stream: put back what was there"""
    from ytvln import ops
    seed, glob = ops.DropoutState.seed, dict(ops.DropoutState._global)
    yield ops.DropoutState
    ops.DropoutState.seed = seed
    ops.DropoutState._global.clear()
    ops.DropoutState._global.update(glob)


def case_inputs(g, case, dev):
    return {k: torch.from_numpy(g[f"{case}_{k}"]).to(dev) for k in ("tokens", "mask", "p", "rnd", "choice")}


def make_inputs(items, group, seed, density=0.2, cap=None, rate=1.5):
    """generated inputs: random words, ~density action ids, a random 0/1 mask, choices that also fall outside [0, n)"""
    rs = np.random.RandomState(seed)
    tokens = rs.randint(1000, V, size=(items, group)).astype(np.int64)
    for bad in R.ACTION_TOKEN_IDS + (R.MASK_TOKEN_ID,):
        tokens[tokens == bad] = bad + 1
    act = rs.rand(items, group) < density
    tokens[act] = np.asarray(R.ACTION_TOKEN_IDS)[rs.randint(0, 3, size=int(act.sum()))]
    mask = (rs.rand(items, group) < 0.7).astype(np.int64)
    p = rs.rand(items, group).astype(np.float32)
    rnd = rs.randint(0, V, size=(items, group)).astype(np.int64)
    nmax = int(act.sum(1).max())
    cap = int(rate * nmax) + 2 if cap is None else cap
    choice = rs.randint(-2, nmax + 3, size=(items, max(cap, 1))).astype(np.int64)[:, :cap]
    return tokens, mask, p, rnd, choice


def run_explicit(dev, tokens, mask, p, rnd, choice, rate, items, **kw):
    from ytvln import batch as B
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    out, tgt, counts = B.randomize_tokens(t(tokens), t(mask), p=t(p), random_tokens=t(rnd), action_choice=t(choice), mask_action_rate=rate,
                                          items=items, return_counts=True, **kw)
    return out.cpu().numpy(), tgt.cpu().numpy(), counts.cpu().numpy()


# ---- 1. the reference's outputs, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_explicit_draws_match_the_reference_golden(dev, lib, case):
    g = gold("g22_action_masking.npz")
    items, group = CASES[case]
    k = lambda name: g[f"{case}_{name}"]  # noqa: E731
    rate = float(k("rate"))
    out, tgt, counts = run_explicit(dev, k("tokens"), k("mask"), k("p"), k("rnd"), k("choice"), rate, None)     # 3-D: items = shape[0]
    assert out.dtype == np.int64 and out.shape == k("tokens").shape
    assert np.array_equal(counts, k("counts")), (counts.tolist(), k("counts").tolist())
    assert np.array_equal(out, k("out")) and np.array_equal(tgt, k("tgt"))
    # the switch: a position drawn more than once keeps the word as its target
    out2, tgt2, counts2 = run_explicit(dev, k("tokens"), k("mask"), k("p"), k("rnd"), k("choice"), rate, items, repeat_target="token")
    want = R.randomize_tokens_action(k("tokens"), k("mask"), k("p"), k("rnd"), k("choice"), rate, items, repeat_target="token")
    assert np.array_equal(out2, want[0]) and np.array_equal(tgt2, want[1]) and np.array_equal(counts2, want[2])
    assert np.array_equal(out2, out) and not bool((tgt2 == R.MASK_TOKEN_ID).any())
    if case == "c":
        assert not np.array_equal(tgt2, tgt)            # repeats are certain there


# ---- 2. rate 0 ------------------------------------------------------------------------------------------------------------------------------
def test_rate_zero_is_the_plain_kernel(dev, lib, stream_state):
    from ytvln import batch as B, ops
    g = gold("g7_masking.npz")
    t = lambda k: torch.from_numpy(g[k]).to(dev)  # noqa: E731
    out, tgt, counts = B.randomize_tokens(t("tokens"), t("mask"), p=t("p_tok"), random_tokens=t("rnd_tok"), items=14, return_counts=True)
    assert torch.equal(out, t("out_tok")) and torch.equal(tgt, t("tgt_tok"))              # the new entry point (it returns the counts)
    assert counts.shape == (14, 2) and bool((counts[:, 1] == 0).all())
    out, tgt = B.randomize_tokens(t("tokens"), t("mask"), p=t("p_tok"), random_tokens=t("rnd_tok"), mask_action_rate=0.0)
    assert torch.equal(out, t("out_tok")) and torch.equal(tgt, t("tgt_tok"))              # the keyword default: the old entry point
    # Philox: the per-token draws of the new kernel sit where the plain kernel's do
    stream_state.manual_seed(77)
    ops.DropoutState(dev)
    st = stream_state.get_state()
    plain = B.randomize_tokens(t("tokens"), t("mask"))
    stream_state.set_state(st, device=dev)
    new = B.randomize_tokens(t("tokens"), t("mask"), items=14, return_counts=True)
    assert torch.equal(plain[0], new[0]) and torch.equal(plain[1], new[1])
    assert int((plain[1] != -1).sum()) > 20


# ---- 3. edges -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 63, 64, 65, 257, 1024, 8192])
def test_explicit_draws_edge_sizes(dev, lib, group):
    """one token, around a wave, around a 256-token chunk, several chunks, the limit; the choices include values outside [0, n)"""
    items = 3
    ins = make_inputs(items, group, seed=group, density=0.6 if group == 1 else 0.2)
    for rep in ("reference", "token"):
        got = run_explicit(dev, *ins, 1.5, items, repeat_target=rep)
        want = R.randomize_tokens_action(*ins, 1.5, items, repeat_target=rep)
        for a, b, what in zip(got, want, ("out", "targets", "counts")):
            assert np.array_equal(a, b), (group, rep, what, int((a != b).sum()))
    if group >= 63:          # the inputs exercise what they are meant to: action words in every item, repeats (a [MASK] target) somewhere
        want = R.randomize_tokens_action(*ins, 1.5, items, repeat_target="reference")
        assert int(want[2][:, 0].min()) > 0 and bool((want[1] == R.MASK_TOKEN_ID).any())


def test_explicit_draws_cap_and_out_of_range(dev, lib):
    items, group = 4, 300
    tokens, mask, p, rnd, choice = make_inputs(items, group, seed=5, cap=3, rate=1.0)
    got = run_explicit(dev, tokens, mask, p, rnd, choice, 1.0, items)                   # cap < m: only cap draws are read
    want = R.randomize_tokens_action(tokens, mask, p, rnd, choice, 1.0, items)
    assert bool((want[2][:, 1] > 3).all())
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert int(((got[0] != tokens) & np.isin(tokens, R.ACTION_TOKEN_IDS) & (mask == 0)).sum()) <= 3 * items
    # nothing but out-of-range choices: no draw at all, i.e. the plain rule (with (n, m) still reported)
    wild = np.where(np.arange(8)[None, :] % 2 == 0, -1 - np.arange(8)[None, :], 10 ** 12 + np.arange(8)[None, :]).repeat(items, 0).astype(np.int64)
    wild[:, 3] = want[2][:, 0]                                                             # n itself is out of range
    got = run_explicit(dev, tokens, mask, p, rnd, wild, 1.0, items)
    plain = R.randomize_tokens_action(tokens, mask, p, rnd, None, 0.0, items)
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1]) and np.array_equal(got[2], want[2])


# ---- 4. Philox: everything else is untouched -----------------------------------------------------------------------------------------------
def test_philox_differs_from_the_plain_call_only_at_action_positions(dev, lib, stream_state):
    from ytvln import batch as B, ops
    tokens, mask, _, _, _ = make_inputs(6, 560, seed=11, density=0.1)
    tok, msk = torch.from_numpy(tokens).to(dev).view(6, 7, 80), torch.from_numpy(mask).to(dev).view(6, 7, 80)
    stream_state.manual_seed(2024)
    ops.DropoutState(dev)
    st = stream_state.get_state()
    plain_out, plain_tgt = B.randomize_tokens(tok, msk)
    stream_state.set_state(st, device=dev)
    out, tgt, counts = B.randomize_tokens(tok, msk, mask_action_rate=0.5, return_counts=True)
    diff = (out != plain_out) | (tgt != plain_tgt)
    is_action = torch.from_numpy(np.isin(tokens, R.ACTION_TOKEN_IDS)).to(dev).view_as(tok)
    assert int(diff.sum()) > 0 and not bool((diff & ~is_action).any())
    assert bool((out[diff] == R.MASK_TOKEN_ID).all())
    assert bool(((tgt[diff] == tok[diff]) | (tgt[diff] == R.MASK_TOKEN_ID)).all())
    n = torch.from_numpy(np.isin(tokens, R.ACTION_TOKEN_IDS).sum(1)).to(dev)
    assert torch.equal(counts[:, 0], n) and torch.equal(counts[:, 1], n // 2)
    forced = is_action & (out == R.MASK_TOKEN_ID) & (msk == 0)                             # under mask == 0 only the action step masks
    assert bool((forced.view(6, -1).sum(1) <= counts[:, 1]).all()) and int(forced.sum()) > 0
    assert int((plain_tgt != -1).sum()) > 100                                              # the BERT draw is there, and shared


# ---- 5. Philox: the distribution of the draws ----------------------------------------------------------------------------------------------
def test_philox_draw_distribution(dev, lib, stream_state):
    from ytvln import batch as B, ops
    items, T, n, m = 512, 64, 10, 5
    rs = np.random.RandomState(3)
    tokens = rs.randint(1000, V, size=(items, T)).astype(np.int64)
    for bad in R.ACTION_TOKEN_IDS + (R.MASK_TOKEN_ID,):
        tokens[tokens == bad] = bad + 1
    for it in range(items):
        tokens[it, rs.choice(T, n, replace=False)] = np.asarray(R.ACTION_TOKEN_IDS)[rs.randint(0, 3, size=n)]
    tok = torch.from_numpy(tokens).to(dev).view(items, 1, T)
    msk = torch.zeros_like(tok)                                    # the plain rule does nothing: out == 103 exactly at the drawn positions
    stream_state.manual_seed(31337)
    ops.DropoutState(dev)
    st = stream_state.get_state()
    out, tgt, counts = B.randomize_tokens(tok, msk, mask_action_rate=0.5, return_counts=True)
    assert counts.cpu().tolist() == [[n, m]] * items
    drawn = (out == R.MASK_TOKEN_ID).view(items, T).cpu().numpy()
    tg = tgt.view(items, T).cpu().numpy()
    assert not bool((drawn & ~np.isin(tokens, R.ACTION_TOKEN_IDS)).any())
    assert np.array_equal(out.view(items, T).cpu().numpy()[~drawn], tokens[~drawn]) and bool((tg[~drawn] == -1).all())
    assert bool(np.isin(tg[drawn], (R.MASK_TOKEN_ID,) + R.ACTION_TOKEN_IDS).all())
    distinct = drawn.sum(1)
    assert distinct.min() >= 1 and distinct.max() <= m
    total, mean, sigma = int(distinct.sum()), items * n * (1 - 0.9 ** m), 35.2
    print(f"drawn positions {total} (expected {mean:.1f}, sigma {sigma})")
    assert abs(total - mean) < 4 * sigma, total
    per_ord = np.zeros(n, np.int64)
    for it in range(items):
        per_ord += drawn[it][R.action_positions(tokens[it])]
    print("items in which each ordinal is hit:", per_ord.tolist())
    assert bool((np.abs(per_ord - 209.7) <= 50).all()), per_ord.tolist()
    assert bool(((tg == R.MASK_TOKEN_ID).sum(1) <= m - distinct).all())           # a repeat costs at least one distinct position
    full = distinct == m                                                          # five distinct positions: no repeat anywhere
    assert bool((tg[full][drawn[full]] == tokens[full][drawn[full]]).all())
    out2, _ = B.randomize_tokens(tok, msk, mask_action_rate=0.5)
    assert not torch.equal(out2, out)                                             # the device-side counter advanced
    stream_state.set_state(st, device=dev)
    out3, tgt3 = B.randomize_tokens(tok, msk, mask_action_rate=0.5)
    assert torch.equal(out3, out) and torch.equal(tgt3, tgt)


# ---- 6. mask_batch ---------------------------------------------------------------------------------------------------------------------------
def test_mask_batch_with_action_rate(dev, lib, stream_state):
    import types
    from ytvln import batch as B, ops, synth
    bs, K, T = 3, 7, 80
    nb = synth.make_batch(bs=bs, K=K, T=T, frames=2, boxes=4, F=64, C=21, seed=5, ignore_rank_frac=0.0)
    rs = np.random.RandomState(8)
    tokens = np.where(nb[8] != -1, nb[8], nb[6])                  # undo the generator's own masking
    for bad in R.ACTION_TOKEN_IDS + (R.MASK_TOKEN_ID,):
        tokens[tokens == bad] = bad + 1
    plant = (rs.rand(bs, K, T) < 0.1) & (nb[7] != 0)
    tokens[plant] = np.asarray(R.ACTION_TOKEN_IDS)[rs.randint(0, 3, size=int(plant.sum()))]
    tokens[1, 5:] = 0                                             # padded options: all-zero rows
    nb[6], nb[7] = tokens, (tokens > 0).astype(nb[7].dtype)
    fresh = lambda: [a.clone() for a in synth.to_torch(nb, dev)]  # noqa: E731  (features are masked in place)
    is_action = torch.from_numpy(np.isin(tokens, R.ACTION_TOKEN_IDS)).to(dev)
    stream_state.manual_seed(99)
    ops.DropoutState(dev)
    st = stream_state.get_state()

    b0 = fresh()
    today = B.mask_batch(b0)
    stream_state.set_state(st, device=dev)
    b1 = fresh()
    again = B.mask_batch(b1, masked_language=True, masked_vision=True, mask_action_rate=0.0, args=None)
    for i, (x, y) in enumerate(zip(today, again)):
        assert torch.equal(x, y), i                               # the defaults are today's mask_batch

    stream_state.set_state(st, device=dev)
    b2 = fresh()
    got = B.mask_batch(b2, args=types.SimpleNamespace(mask_action_rate=0.5, masked_language=True, masked_vision=True))
    for i in (1, 4, 5):
        assert torch.equal(got[i], today[i]), i                   # the region masking does not move
    diff = (got[6] != today[6]) | (got[8] != today[8])
    assert int(diff.sum()) > 0 and not bool((diff & ~is_action).any())
    n_item = is_action.view(bs, -1).sum(1)
    forced = diff.view(bs, -1).sum(1)
    assert bool((forced >= 1).all()) and bool((forced <= n_item // 2).all())              # the action share: up to int(0.5 * n) per item
    assert bool((got[6][diff] == R.MASK_TOKEN_ID).all())
    assert bool((got[8][1, 5:] == -1).all()) and bool((got[6][1, 5:] == 0).all())         # padded options: no targets

    stream_state.set_state(st, device=dev)
    b3 = fresh()
    keep = [a.clone() for a in b3]
    off = B.mask_batch(b3, masked_language=False, masked_vision=False, mask_action_rate=0.5)
    assert torch.equal(off[6], keep[6]) and bool((off[8] == -1).all()) and off[8].shape == keep[6].shape and off[8].dtype == torch.int64
    assert torch.equal(off[1], keep[1]) and off[1].data_ptr() == b3[1].data_ptr()
    assert torch.equal(off[4], torch.ones_like(keep[4]) / 21) and off[5].shape == keep[3].shape and not bool(off[5].any())
    assert off[5].dtype == keep[3].dtype


# ---- 7. graph capture ------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_with_refilled_inputs(dev, lib):
    from ytvln import batch as B
    g = gold("g22_action_masking.npz")
    first = case_inputs(g, "a", dev)
    second = {k: v.flip(0).contiguous() for k, v in first.items()}            # the items in another order
    rate = float(g["a_rate"])

    def run(x):
        return B.randomize_tokens(x["tokens"], x["mask"], p=x["p"], random_tokens=x["rnd"], action_choice=x["choice"], mask_action_rate=rate,
                                  return_counts=True)

    eager = [[o.clone() for o in run(f)] for f in (first, second)]
    assert torch.equal(eager[0][0], torch.from_numpy(g["a_out"]).to(dev)) and torch.equal(eager[1][0], eager[0][0].flip(0))
    x = {k: v.clone() for k, v in first.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(x)                        # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(x)
    for f, want in ((second, eager[1]), (first, eager[0])):
        for k in x:
            x[k].copy_(f[k])
        graph.replay()
        torch.cuda.synchronize()
        for got, w in zip(outs, want):
            assert torch.equal(got, w)
