"""Statement of what ytvln_expand_ragged_masked / ytvln_expand_records_masked compute (include/ytvln.h), on the CPU, shared by
test_pool_masked_cpu.py and test_pool_masked_gpu.py: the existing statement of the expansion (ragged_pool_ref / record_pool_ref), then the
oracle's randomize_regions with explicit draws, then torch's rounding to bfloat16 for the bf16 feature output.  Also the inputs of those
tests: pool features with the bit patterns that tell bf16 roundings apart, and draws that visit every decision class and both thresholds."""
import functools

import numpy as np
import torch

import vilbert_ref as O
from ragged_pool_ref import expand_ragged_ref, grid_pool
from record_pool_ref import expand_records_ref, grid_records

BOXES = 6
GRID = [(64, 21), (2048, 1601), (6, 1601), (5, 21)]
BIG = dict(boxes=37, frames=2, bs=1, K=2, F=2048, C=1601)          # ten pieces of four rows (the last of one) per slot
SHAPES = [("grid", F, C) for F, C in GRID] + [("big", BIG["F"], BIG["C"])]

T_MASK = np.float32(0.85)                         # the kernels' thresholds: the reference's Python doubles rounded to fp32
T_ZERO = np.float32(0.85 + 0.15 * 0.1)


def _below(x):
    return np.nextafter(np.float32(x), np.float32(0))


# the draws of consecutive real rows, cycled: below 0.85 / two selected in a row / two zeroed in a row / both thresholds exactly and one ulp below
PHASES = np.array([0.3, 0.855, 0.86, 0.9, 0.95, 0.1, T_MASK, _below(T_MASK), T_ZERO, _below(T_ZERO), 0.5, 0.2, 0.7], np.float32)
PADDED_DRAW = np.float32(0.99)                    # on every row behind a zero mask: must change nothing

# fp32 bit patterns whose rounding to bf16 tells round-to-nearest-even from truncation and from round-half-up: low half 0x7FFF, a tie under
# an even and under an odd upper half, 0x8001, a round-up into the next binade, the same negative, both zeros
BF16_PATTERNS = np.array([0x3F807FFF, 0x3F808000, 0x3F818000, 0x3F808001, 0x3F7FFFFF, 0xBF808000, 0xBF818000, 0xBF808001, 0xC0A07FFF, 0x00000000,
                          0x80000000], np.uint32)


def plant_patterns(pf):
    """Every third value of the pool features becomes one of BF16_PATTERNS, in turn (in place; returns pf)."""
    flat = pf.reshape(-1).view(np.uint32)
    at = np.arange(0, flat.size, 3)
    flat[at] = BF16_PATTERNS[np.arange(at.size) % len(BF16_PATTERNS)]
    return pf


def make_draws(mask):
    """fp32 draws of the shape of `mask`: PHASES in turn over the real rows in flat order, PADDED_DRAW everywhere else."""
    p = np.full(mask.shape, PADDED_DRAW, np.float32)
    real = np.flatnonzero(mask.reshape(-1))
    p.reshape(-1)[real] = PHASES[np.arange(real.size) % len(PHASES)]
    return p


def masked_ref(expanded, p, bf16=False):
    """(features, boxes, probs, masks) of expand_*_ref (numpy) and the draws p (numpy fp32, or None = masking off) -> the five outputs of the
    fused expansion as CPU tensors."""
    f, bx, pr, m = (torch.from_numpy(a) for a in expanded[:4])
    if p is None:
        tg, tm = torch.ones_like(pr) / pr.shape[-1], torch.zeros_like(m)
    else:
        f, tg, tm = O.randomize_regions(f, pr, m, torch.from_numpy(p))
    return (f.to(torch.bfloat16) if bf16 else f), bx, tg, m, tm


def _big_index():
    index = np.array([[[5, 3], [4, -1]]], np.int64)          # frames of boxes+3 (cut), boxes, boxes+1 rows (ragged) and a padding frame
    assert index.shape == (BIG["bs"], BIG["K"], BIG["frames"])
    return index


@functools.lru_cache(maxsize=None)
def ragged_case(kind, F, C):
    """(boxes, numpy inputs (pf, pl, pp, offsets, index), unmasked statement, draws) of one shape; computed once, never modified."""
    boxes = BOXES if kind == "grid" else BIG["boxes"]
    pf, pl, pp, offsets, index = grid_pool(boxes, F, C)
    plant_patterns(pf)
    if kind == "big":
        index = _big_index()
    inp = (pf, pl, pp, offsets, index)
    ref = expand_ragged_ref(*inp, boxes)
    assert ref[4] == 0
    return boxes, inp, ref[:4], make_draws(ref[3])


@functools.lru_cache(maxsize=None)
def records_case(kind, F, C, with_view):
    """(boxes, numpy inputs (pf, pg, pp, offsets, index, view), unmasked statement, draws) of one shape, with or without `view`."""
    boxes = BOXES if kind == "grid" else BIG["boxes"]
    pf, pg, pp, offsets, index, view = grid_records(boxes, F, C)
    plant_patterns(pf)
    if kind == "big":
        index = _big_index()
        view = np.random.RandomState(3).uniform(-np.pi, np.pi, index.shape + (2,))
    inp = (pf, pg, pp, offsets, index, view)
    ref = expand_records_ref(*inp[:5], boxes, view if with_view else None)
    assert ref[4] == 0
    return boxes, inp, ref[:4], make_draws(ref[3])
