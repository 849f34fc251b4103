"""On-device batch preparation: the masking the reference's datasets apply per item on the host
(`utils/dataset/common.py:213-300`, called from `utils/dataset/all_dataset.py`), done for a whole `[bs, K, ...]` batch that already
sits in HBM.  The loader then only has to ship the un-masked tokens / features / class probabilities once.

    randomize_tokens(tokens, mask)                   -> (tokens, targets)                  common.py:213-270
    randomize_tokens(tokens, mask, mask_action_rate=r) the same with `--mask_action_rate r`  common.py:234-253   (per dataset item)
    randomize_regions(features, probs, mask)         -> (features, targets, targets_mask)  common.py:272-300   (features in place)
    mask_batch(batch, args=args)                     -> the 16-tuple with items 1, 4, 5, 6, 8 replaced

Draws come from the library's Philox stream (`ops.DropoutState`: seed + device-side counter, so the masks change every call and
replay inside a hipGraph); passing `p=` / `random_tokens=` (/ `action_choice=`) reproduces the reference functions bit for bit (tests).

Action-aware masking (`mask_action_rate` > 0): per item, int(rate * n) of the n occurrences of 'left' / 'forward' / 'right' are drawn
with replacement and always become `[MASK]` targets, on top of the 15 % BERT draw.  The reference reads back its own writes while it
applies the draws, so a position drawn twice gets the `[MASK]` id as its TARGET; its checkpoints were trained that way and
`repeat_target="reference"` (default) reproduces it, `repeat_target="token"` keeps the word.  Rate 0 is the plain kernel, unchanged.
"""
from __future__ import annotations

import math
import struct
from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import ops
from ._lib import call

MASK_TOKEN_ID = 103         # tokenizer.vocab["[MASK]"] of bert-base-uncased (common.py:255)
VOCAB_SIZE = 30522          # len(tokenizer.vocab)
ACTION_TOKEN_IDS = (2187, 2830, 2157)   # 'left', 'forward', 'right' (common.py:216-221, 235): the order of the reference's enumeration
MAX_ACTION_RATE = 16.0      # guard on the kernel's draw loop (the paper uses at most 1); ACT_MAX_RATE of csrc/batch.hip
MAX_ACTION_GROUP = 8192     # tokens per item the action kernel holds hit counts for in LDS; ACT_MAX_GROUP of csrc/batch.hip


def _dev(t: Tensor, name: str) -> Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"ytvln.batch: `{name}` must live on the GPU (no CPU path)")
    return t.contiguous()


def _check_action_args(rate, action_tokens) -> Tuple[float, Tuple[int, int, int]]:
    try:
        rate = float(rate)
    except (TypeError, ValueError):
        raise ValueError(f"ytvln.batch: mask_action_rate must be a number, got {rate!r}") from None
    if not math.isfinite(rate) or rate < 0.0 or rate > MAX_ACTION_RATE:
        raise ValueError(f"ytvln.batch: mask_action_rate must be finite and within [0, {MAX_ACTION_RATE:g}], got {rate!r}")
    try:
        ids = tuple(int(a) for a in action_tokens)
    except (TypeError, ValueError):
        raise ValueError(f"ytvln.batch: action_tokens must be three distinct token ids, got {action_tokens!r}") from None
    if len(ids) != 3 or len(set(ids)) != 3 or any(a != b for a, b in zip(ids, action_tokens)):
        raise ValueError(f"ytvln.batch: action_tokens must be three distinct integer token ids, got {action_tokens!r}")
    return rate, ids


def randomize_tokens(tokens: Tensor, mask: Tensor, vocab_size: int = VOCAB_SIZE, mask_token_id: int = MASK_TOKEN_ID,
                     p: Optional[Tensor] = None, random_tokens: Optional[Tensor] = None, mask_action_rate: float = 0.0,
                     items: Optional[int] = None, action_tokens: Sequence[int] = ACTION_TOKEN_IDS, action_choice: Optional[Tensor] = None,
                     repeat_target: str = "reference", return_counts: bool = False):
    """`mask_action_rate` > 0 (the reference's `--mask_action_rate`, common.py:234-253): the tensor is `items` dataset items of K*T
    contiguous tokens each (default `tokens.shape[0]` for >= 3 dimensions) and, per item, int(rate * n) of its n action words are drawn with
    replacement and always become `[MASK]` targets.  `repeat_target`: the target of a position drawn more than once -- "reference": the
    `[MASK]` id, which is what the reference computes; "token": the word.  `action_choice` int64 [items, cap] supplies the drawn
    ordinals next to explicit `p` / `random_tokens` (tests).  `return_counts` adds an int64 [items, 2] tensor of (n, m) per item."""
    rate, ids = _check_action_args(mask_action_rate, action_tokens)
    if repeat_target not in ("reference", "token"):
        raise ValueError(f"ytvln.batch: repeat_target is 'reference' or 'token', got {repeat_target!r}")
    explicit = p is not None and random_tokens is not None
    if rate > 0.0 or return_counts:
        if items is None:
            if tokens.dim() < 3:
                raise ValueError("ytvln.batch: with mask_action_rate, `items` must be given for tensors of fewer than 3 dimensions "
                                 "(the action draw is per dataset item: all K instructions of an item together)")
            items = tokens.shape[0]
        items = int(items)
        if items < 1 or tokens.numel() % items != 0 or tokens.numel() == 0:
            raise ValueError(f"ytvln.batch: items = {items} does not divide a tensor of {tokens.numel()} tokens")
        if tokens.numel() // items > MAX_ACTION_GROUP:
            raise ValueError(f"ytvln.batch: {tokens.numel() // items} tokens per item exceed the kernel's limit of {MAX_ACTION_GROUP}")
        if mask.numel() != tokens.numel():
            raise ValueError(f"ytvln.batch: mask {tuple(mask.shape)} does not match tokens {tuple(tokens.shape)}")
        if explicit and rate > 0.0 and action_choice is None:
            raise ValueError("ytvln.batch: explicit `p` / `random_tokens` with mask_action_rate need `action_choice` as well")
        if action_choice is not None and (not explicit or action_choice.dim() != 2 or action_choice.shape[0] != items):
            raise ValueError("ytvln.batch: `action_choice` is [items, cap] and goes with explicit `p` and `random_tokens`")
    elif action_choice is not None:
        raise ValueError("ytvln.batch: `action_choice` without mask_action_rate")
    tokens = _dev(tokens, "tokens").long()
    mask = _dev(mask, "mask").long()
    out, targets = torch.empty_like(tokens), torch.empty_like(tokens)
    st = None if explicit else ops.DropoutState(tokens.device)
    p = _dev(p, "p").float() if explicit else None
    random_tokens = _dev(random_tokens, "random_tokens").long() if explicit else None
    p_ptr, r_ptr = ops._ptr(p), ops._ptr(random_tokens)
    if rate == 0.0 and not return_counts:           # today's entry point: same bits, same launches
        call("ytvln_randomize_tokens", ops._ptr(tokens), ops._ptr(mask), tokens.numel(), int(vocab_size), int(mask_token_id), p_ptr, r_ptr,
             None if explicit else ops._ptr(st.tensor), 0 if explicit else st.next_site(), ops._ptr(out), ops._ptr(targets), ops._stream())
        return out, targets
    choice = _dev(action_choice, "action_choice").long() if action_choice is not None else None
    cap = choice.shape[1] if choice is not None else 0
    counts = torch.empty(items, 2, dtype=torch.int64, device=tokens.device) if return_counts else None
    site = 0 if explicit else st.next_site()        # the per-token draws sit where the plain call puts them
    action_site = 0 if explicit else st.next_site()
    call("ytvln_randomize_tokens_action", ops._ptr(tokens), ops._ptr(mask), items, tokens.numel() // items, int(vocab_size), int(mask_token_id),
         ids[0], ids[1], ids[2], struct.unpack("<q", struct.pack("<d", rate))[0], 1 if repeat_target == "reference" else 0, p_ptr, r_ptr,
         ops._ptr(choice) if cap else None, cap, None if explicit else ops._ptr(st.tensor), site, action_site, ops._ptr(out), ops._ptr(targets),
         ops._ptr(counts) if return_counts else None, ops._stream())
    return (out, targets, counts) if return_counts else (out, targets)


def randomize_regions(features: Tensor, probs: Tensor, mask: Tensor, p: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """`features` ([..., F], fp32, unit inner stride) is modified IN PLACE like the reference does (`features[p >= thresh] = 0`)."""
    if not (features.is_cuda and features.dtype == torch.float32 and features.is_contiguous()):
        raise RuntimeError("ytvln.batch: `features` must be a contiguous fp32 GPU tensor (it is masked in place)")
    probs = _dev(probs, "probs").float()
    mask = _dev(mask, "mask").long()
    F, C = features.shape[-1], probs.shape[-1]
    rows = mask.numel()
    assert features.numel() == rows * F and probs.numel() == rows * C, (features.shape, probs.shape, mask.shape)
    targets = torch.empty_like(probs)
    tmask = torch.empty_like(mask)
    st = None if p is not None else ops.DropoutState(features.device)
    call("ytvln_randomize_regions", ops._ptr(features), F, ops._ptr(probs), ops._ptr(mask), rows, F, C,
         ops._ptr(_dev(p, "p").float()) if p is not None else None, None if p is not None else ops._ptr(st.tensor),
         0 if p is not None else st.next_site(), ops._ptr(targets), ops._ptr(tmask), ops._stream())
    return features, targets, tmask


def expand_options(pool_features: Tensor, pool_boxes: Tensor, pool_probs: Tensor, pool_masks: Tensor, index: Tensor):
    """Option expansion on the device.  The reference materialises K options per item on the host -- the positive path, caption
    negatives that SHARE its features, frame permutations of it and paths with some frames swapped for random photos
    (`utils/dataset/all_dataset.py:185-233`, `common.py:430-522`) -- and ships all K copies (132 MB of features per step at
    BASELINE config 2).  Here the loader ships each distinct frame once:

        pool_features [P, boxes, F]   pool_boxes [P, boxes, 12]   pool_probs [P, boxes, C]   pool_masks [P, boxes]  (one entry per frame)
        index         [bs, K, frames] int64: the pool entry shown at each position of each option, -1 = padding frame

    and the [bs, K, frames*boxes, ...] tensors of the 16-tuple are gathered in HBM (column 11 of the boxes = the position of the
    frame inside the option, `all_dataset.py:314`).  Returns (image_features, image_boxes, image_probs, image_masks)."""
    bs, K, frames = index.shape
    P, boxes = pool_masks.shape
    idx = _dev(index, "index").long().reshape(-1)
    n = idx.numel()
    feats = ops.gather_rows(_dev(pool_features, "pool_features").reshape(P, -1), idx).view(bs, K, frames * boxes, -1)
    bx = ops.gather_rows(_dev(pool_boxes, "pool_boxes").reshape(P, -1), idx).view(bs, K, frames, boxes, -1)
    valid = (idx >= 0).view(bs, K, frames, 1)
    pos = torch.arange(frames, device=idx.device, dtype=bx.dtype).view(1, 1, frames, 1).expand(bs, K, frames, boxes)
    bx[..., 11] = torch.where(valid.expand(bs, K, frames, boxes), pos, torch.zeros_like(pos))
    probs = ops.gather_rows(_dev(pool_probs, "pool_probs").reshape(P, -1), idx).view(bs, K, frames * boxes, -1)
    masks = (_dev(pool_masks, "pool_masks").long()[idx.clamp(min=0)] * (idx >= 0).view(n, 1)).view(bs, K, frames * boxes)
    return feats, bx.view(bs, K, frames * boxes, -1), probs, masks


def mask_batch(batch: Sequence[Tensor], vocab_size: int = VOCAB_SIZE, mask_token_id: int = MASK_TOKEN_ID, masked_language: bool = True,
               masked_vision: bool = True, mask_action_rate: float = 0.0, args=None) -> List[Tensor]:
    """Apply both maskings to an un-masked device batch in the 16-tuple layout of `get_model_input` (utils/utils_init.py:34-53):
    1 image_features, 3 image_masks, 4 image_targets (class probabilities in, MVM targets out), 5 image_targets_mask (out),
    6 instr_tokens [bs, K, T], 7 instr_mask, 8 instr_targets (out).

    `masked_language` / `masked_vision` / `mask_action_rate` are the reference's options of the same names; `args` (the parsed command
    line) supplies all three when given.  A disabled masking returns what the reference's dataset returns (`all_dataset.py:251-261`):
    instr_targets = -1, or image_targets = 1/C with a zero image_targets_mask, and the inputs untouched.  The action draw is per
    dataset item, i.e. per row of the batch dimension: all K instructions of an item together, like the reference."""
    if args is not None:
        masked_language = bool(getattr(args, "masked_language", masked_language))
        masked_vision = bool(getattr(args, "masked_vision", masked_vision))
        mask_action_rate = getattr(args, "mask_action_rate", mask_action_rate)
    rate, _ = _check_action_args(mask_action_rate, ACTION_TOKEN_IDS)
    b = list(batch)
    if masked_language:
        b[6], b[8] = randomize_tokens(b[6], b[7], vocab_size, mask_token_id, mask_action_rate=rate)
    else:
        b[8] = torch.full_like(b[6], -1)
    if masked_vision:
        b[1], b[4], b[5] = randomize_regions(b[1], b[4], b[3])
    else:
        b[4], b[5] = torch.ones_like(b[4]) / b[4].shape[-1], torch.zeros_like(b[3])
    return b
