"""CPU: action-aware token masking (`mask_action_rate`, utils/dataset/common.py:234-253) -- the numpy restatement against the golden
made by running the reference, the draw count in double precision, and every rejection that happens before the GPU is touched."""
import math
import struct

import numpy as np
import pytest
import torch

import action_masking_ref as R
from helpers import gold

CASES = {"a": (5, 300), "b": (4, 560), "c": (3, 24), "d": (2, 128)}


def bits(rate):
    return struct.unpack("<q", struct.pack("<d", rate))[0]


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_reproduces_the_reference(case):
    g = gold("g22_action_masking.npz")
    items, group = CASES[case]
    k = lambda name: g[f"{case}_{name}"]  # noqa: E731
    assert k("tokens").shape[0] == items and k("tokens")[0].size == group
    out, tgt, counts = R.randomize_tokens_action(k("tokens"), k("mask"), k("p"), k("rnd"), k("choice"), float(k("rate")), items)
    assert np.array_equal(out, k("out")) and np.array_equal(tgt, k("tgt")) and np.array_equal(counts, k("counts"))


def test_golden_holds_the_situations_the_tests_rely_on():
    g = gold("g22_action_masking.npz")
    assert g["d_counts"].tolist() == [[10, 7], [0, 0]]                       # 0.7 * 10 in double
    assert [1, 2] in g["c_counts"].tolist() and bool((g["c_counts"][:, 1] > g["c_counts"][:, 0]).all())      # m > n
    assert any(n > 0 and m == 0 for n, m in g["a_counts"].tolist())
    for case, (items, group) in CASES.items():
        flat = g[f"{case}_tokens"].reshape(items, group)[0]
        for pos in (0, 63, 64, 255, 256, group - 1):
            if pos < group and not (case == "d" and pos in (255, 256)):
                assert flat[pos] in R.ACTION_TOKEN_IDS, (case, pos)
    # the quirk is in the data: a target that is the [MASK] id
    assert any(bool((g[f"{c}_tgt"] == R.MASK_TOKEN_ID).any()) for c in CASES)


def test_draw_count_is_a_double_product_truncated():
    assert R.draw_count(0.7, 10) == 7 and int(float(np.float32(0.7)) * 10) == 6      # a rate that crossed the ABI as fp32 would lose a draw
    assert R.draw_count(0.29, 100) == 28
    assert R.draw_count(0.3, 1) == 0
    assert R.draw_count(2.5, 6) == 15 and R.draw_count(1.0, 0) == 0


def test_wrapper_rejects_bad_arguments_before_the_gpu():
    from ytvln import batch as B
    assert B.ACTION_TOKEN_IDS == (2187, 2830, 2157)
    tok = torch.zeros(2, 3, 8, dtype=torch.long)
    msk = torch.ones_like(tok)
    for rate in (-0.1, float("nan"), float("inf"), 16.5, "x"):
        with pytest.raises(ValueError, match="mask_action_rate"):
            B.randomize_tokens(tok, msk, mask_action_rate=rate)
    with pytest.raises(ValueError, match="items"):
        B.randomize_tokens(tok.view(6, 8), msk.view(6, 8), mask_action_rate=0.5)          # 2-D: items must be given
    with pytest.raises(ValueError, match="items"):
        B.randomize_tokens(tok.view(-1), msk.view(-1), mask_action_rate=0.5)
    with pytest.raises(ValueError, match="does not divide"):
        B.randomize_tokens(tok, msk, mask_action_rate=0.5, items=5)
    with pytest.raises(ValueError, match="does not divide"):
        B.randomize_tokens(tok, msk, mask_action_rate=0.5, items=0)
    for bad in ((2187, 2830), (2187, 2830, 2187), (2187, 2830, 2157, 1), (2187.5, 2830, 2157), ("left", "forward", "right"), 7):
        with pytest.raises(ValueError, match="action_tokens"):
            B.randomize_tokens(tok, msk, mask_action_rate=0.5, action_tokens=bad)
    with pytest.raises(ValueError, match="repeat_target"):
        B.randomize_tokens(tok, msk, mask_action_rate=0.5, repeat_target="word")
    with pytest.raises(ValueError, match="limit"):
        B.randomize_tokens(torch.zeros(1, 1, 8193, dtype=torch.long), torch.zeros(1, 1, 8193, dtype=torch.long), mask_action_rate=0.5)
    with pytest.raises(ValueError, match="action_choice"):          # explicit per-token draws need the explicit ordinals too
        B.randomize_tokens(tok, msk, mask_action_rate=0.5, p=torch.zeros(2, 3, 8), random_tokens=tok)
    with pytest.raises(ValueError, match="action_choice"):
        B.randomize_tokens(tok, msk, action_choice=torch.zeros(2, 4, dtype=torch.long))
    with pytest.raises(ValueError, match="mask_action_rate"):
        B.mask_batch([tok] * 16, mask_action_rate=-1.0)
    with pytest.raises(ValueError, match="mask_action_rate"):
        B.mask_batch([tok] * 16, args=__import__("types").SimpleNamespace(mask_action_rate=float("nan")))
    with pytest.raises(RuntimeError, match="GPU"):                  # valid arguments: the usual refusal of CPU tensors, no fallback
        B.randomize_tokens(tok, msk, mask_action_rate=0.5)
    with pytest.raises(RuntimeError, match="GPU"):
        B.randomize_tokens(tok, msk)


def test_entry_point_rejects_bad_arguments_without_a_device():
    from ytvln import _lib
    lib = _lib.load()
    assert lib.ytvln_version() == _lib.ABI_VERSION == 2
    assert "ytvln_randomize_tokens_action" in _lib.SIGNATURES and len(_lib.SIGNATURES["ytvln_randomize_tokens_action"]) == 22
    F = 4096         # a non-null address that is never dereferenced: every case below must fail before a launch

    def args(**over):
        a = dict(tokens=F, mask=F, items=2, group=24, vocab=30522, mask_id=103, a0=2187, a1=2830, a2=2157, rate=bits(0.5), repeat=1,
                 p=None, rnd=None, choice=None, cap=0, rng=F, site=1, asite=2, out=F, tgt=F, counts=None, stream=None)
        a.update(over)
        return list(a.values())

    bad = {
        "null buffer": [dict(tokens=None), dict(mask=None), dict(out=None), dict(tgt=None)],
        "overflows": [dict(items=2 ** 62, group=8)],
        "limit": [dict(group=8193), dict(group=2 ** 40)],
        "bad shape": [dict(group=0), dict(items=-1), dict(vocab=0)],
        "rate": [dict(rate=bits(-0.5)), dict(rate=bits(math.nan)), dict(rate=bits(math.inf)), dict(rate=bits(-math.inf)), dict(rate=bits(17.0)),
                 dict(rate=-1)],
        "action ids": [dict(a1=2187), dict(a2=2187), dict(a2=2830)],
        "repeat_target": [dict(repeat=2)],
        "explicit draws": [dict(rng=None), dict(rng=None, p=F), dict(rng=None, rnd=F)],
        "action_choice": [dict(p=F, rnd=F, rng=None, cap=4), dict(p=F, rnd=F, rng=None, choice=F, cap=-1)],
    }
    for what, cases in bad.items():
        for over in cases:
            with pytest.raises(RuntimeError, match=f"ytvln_randomize_tokens_action failed.*{what}"):
                _lib.call("ytvln_randomize_tokens_action", *args(**over))
    _lib.call("ytvln_randomize_tokens_action", *args(items=0))         # nothing to do: success without a launch
