"""On-device batch preparation: the masking the reference's datasets apply per item on the host
(`utils/dataset/common.py:213-300`, called from `utils/dataset/all_dataset.py`), done for a whole `[bs, K, ...]` batch that already
sits in HBM.  The loader then only has to ship the un-masked tokens / features / class probabilities once.

    randomize_tokens(tokens, mask)                   -> (tokens, targets)                  common.py:213-270
    randomize_tokens(tokens, mask, mask_action_rate=r) the same with `--mask_action_rate r`  common.py:234-253   (per dataset item)
    randomize_regions(features, probs, mask)         -> (features, targets, targets_mask)  common.py:272-300   (features in place)
    mask_batch(batch, args=args)                     -> the 16-tuple with items 1, 4, 5, 6, 8 replaced
    expand_options(pool..., index)                   -> items 1, 2, 4, 3 from a pool padded to `boxes` rows per frame
    expand_ragged(pool..., offsets, index, boxes)    -> the same from the un-padded rows the feature readers return, in one launch
    RaggedPool(capacity_rows, capacity_frames)       pinned staging + static device buffers around expand_ragged
    global_rows(pool_features, offsets)              -> the readers' global (mean) feature row of every pool frame, numpy's summation order
    expand_records(pool..., offsets, index, boxes)   -> expand_ragged from RAW records: global region, box geometry, headings on the device
    RecordPool(capacity_rows, capacity_frames)       pinned staging + static device buffers around global_rows + expand_records
    expand_ragged_masked / expand_records_masked     the expansions with randomize_regions, and bf16 features on request, in the same launch
    pool.expand_masked(index, boxes, ...)            -> items 1, 2, 4, 3, 5; then mask_batch(..., vision_premasked=True) for the tokens

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
import warnings
from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import ops
from ._lib import DT_BF16, DT_F32, call

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
    frame inside the option, `all_dataset.py:314`).  Returns (image_features, image_boxes, image_probs, image_masks).

    Column 11 of a PADDING frame (index -1) is 0 here; `expand_ragged` writes the position there as the reference does
    (`all_dataset.py:331`).  The difference is confined to rows behind a zero mask."""
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


def _want(t, name: str, dtype, shape) -> None:
    """ValueError unless `t` is a contiguous tensor of this dtype and shape (None in `shape` = any size)."""
    if not torch.is_tensor(t):
        raise ValueError(f"ytvln.batch: `{name}` must be a tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise ValueError(f"ytvln.batch: `{name}` must be {dtype}, got {t.dtype}")
    if t.dim() != len(shape) or any(w is not None and int(w) != int(g) for w, g in zip(shape, t.shape)):
        raise ValueError(f"ytvln.batch: `{name}` must have shape {list(shape)}, got {list(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"ytvln.batch: `{name}` must be contiguous")


def _check_pool(boxes, pool_features, per_row, pool_probs, offsets, index):
    """The checks expand_ragged and expand_records share on their inputs (ValueError, nothing touched).  `per_row` = [(name, tensor, columns
    or None)]: the fp32 tensors that hold one row per row of `pool_features`.  Returns (boxes, rows, F, C, (bs, K, frames))."""
    boxes = int(boxes)
    if boxes <= 0:
        raise ValueError(f"ytvln.batch: boxes must be positive, got {boxes}")
    _want(pool_features, "pool_features", torch.float32, (None, None))
    rows, F = pool_features.shape
    for name, t, cols in per_row:
        _want(t, name, torch.float32, (rows, cols))
    C = 0
    if pool_probs is not None:
        _want(pool_probs, "pool_probs", torch.float32, (rows, None))
        C = pool_probs.shape[1]
    _want(offsets, "offsets", torch.int64, (None,))
    if offsets.numel() < 1:
        raise ValueError("ytvln.batch: `offsets` holds one entry per pool frame plus one")
    _want(index, "index", torch.int64, (None, None, None))
    if index.shape[2] <= 0:
        raise ValueError("ytvln.batch: `index` [bs, K, frames] needs frames >= 1")
    return boxes, rows, F, C, tuple(index.shape)


def _check_out(who: str, inputs, out, bad, lead, F: int, C: int):
    """The second half of those checks: `out` and `bad` (ValueError), then every tensor on the GPU (RuntimeError) and on one device.
    `inputs` = [(name, tensor or None)], `pool_features` first and `pool_probs` among them; `lead` = (bs, K, frames * boxes).  Returns the
    four output tensors, allocated here when `out` is None."""
    probs = dict(inputs)["pool_probs"] is not None
    if out is not None:
        if len(out) != 4:
            raise ValueError("ytvln.batch: `out` is (image_features, image_boxes, image_probs, image_masks)")
        f, bx, pr, m = out
        _want(f, "out[0]", torch.float32, (*lead, F))
        _want(bx, "out[1]", torch.float32, (*lead, 12))
        if (pr is None) == probs:
            raise ValueError("ytvln.batch: out[2] (image_probs) and `pool_probs` go together: both given or both None")
        if pr is not None:
            _want(pr, "out[2]", torch.float32, (*lead, C))
        _want(m, "out[3]", torch.int64, lead)
    if bad is not None:
        _want(bad, "bad", torch.int64, (1,))
    tensors = list(inputs) + [("bad", bad)] + ([(f"out[{i}]", t) for i, t in enumerate(out)] if out is not None else [])
    for name, t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"ytvln.batch: `{name}` must live on the GPU (no CPU path)")
    dev = inputs[0][1].device
    if any(t is not None and t.device != dev for _, t in tensors):
        raise ValueError(f"ytvln.batch: {who} needs all its tensors on one device")
    if out is None:
        f = torch.empty(*lead, F, dtype=torch.float32, device=dev)
        bx = torch.empty(*lead, 12, dtype=torch.float32, device=dev)
        pr = torch.empty(*lead, C, dtype=torch.float32, device=dev) if probs else None
        m = torch.empty(*lead, dtype=torch.int64, device=dev)
    return f, bx, pr, m


def expand_ragged(pool_features: Tensor, pool_locations: Tensor, pool_probs: Optional[Tensor], offsets: Tensor, index: Tensor, boxes: int,
                  out: Optional[Sequence[Optional[Tensor]]] = None, bad: Optional[Tensor] = None):
    """Padding, masks and option expansion from a RAGGED frame pool in one launch (`ytvln_expand_ragged_f32`).  The pool holds what the
    feature readers return, un-padded: frame p is rows offsets[p] .. offsets[p+1]-1 of

        pool_features [rows, F] fp32   pool_locations [rows, L <= 11] fp32   pool_probs [rows, C] fp32 or None   offsets [frames_in_pool + 1] int64
        index [bs, K, frames] int64: the pool frame shown at each position of each option, -1 = padding frame

    and every frame is padded (or cut) to `boxes` rows the way `utils/dataset/all_dataset.py:294-345` does on the host: real rows copied,
    the rest exact zeros with mask 0, box columns L..10 zero.  Returns (image_features [bs, K, frames*boxes, F], image_boxes [.., 12],
    image_probs [.., C] or None, image_masks [..] int64).  `out=(f, bx, pr, m)` writes into the given contiguous tensors of those shapes
    (the static inputs of a captured step; `pr` None together with `pool_probs`); whatever they held is overwritten.  `bad` (int64 [1] on
    the device) accumulates the slots whose index or offsets were out of range; such a slot is all padding.

    Column 11 of the boxes is the position of the frame inside its option for EVERY row, padding frames included, which is what the
    reference writes (`all_dataset.py:314` and `:331`); `expand_options` writes 0 for padding frames.  The difference is confined to
    rows behind a zero mask.  Shapes and dtypes are checked first (ValueError, nothing touched); there is no CPU path."""
    boxes, rows, F, C, (bs, K, frames) = _check_pool(boxes, pool_features, [("pool_locations", pool_locations, None)], pool_probs, offsets, index)
    L = pool_locations.shape[1]
    if L > 11:
        raise ValueError(f"ytvln.batch: `pool_locations` has {L} columns; the boxes hold 11 next to the position column")
    f, bx, pr, m = _check_out("expand_ragged", [("pool_features", pool_features), ("pool_locations", pool_locations), ("pool_probs", pool_probs),
                                                ("offsets", offsets), ("index", index)], out, bad, (bs, K, frames * boxes), F, C)
    call("ytvln_expand_ragged_f32", ops._ptr(pool_features), ops._ptr(pool_locations), ops._ptr(pool_probs), ops._ptr(offsets),
         offsets.numel() - 1, rows, ops._ptr(index), bs * K * frames, frames, boxes, F, L, C, ops._ptr(f), ops._ptr(bx), ops._ptr(pr),
         ops._ptr(m), ops._ptr(bad), ops._stream())
    return f, bx, pr, m


def global_rows(pool_features: Tensor, offsets: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """The global feature row of every pool frame (`ytvln_pool_global_rows_f32`): out[p] = the fp32 sum of rows offsets[p] .. offsets[p+1]-1
    of `pool_features` [rows, F], taken strictly in row order, divided by fp32(rows of the frame) -- bit for bit what the reference's readers
    compute with `features.mean(axis=0)` (`features_reader.py:170`).  Zero for an empty frame and for offsets out of order or out of range.
    `out` (fp32 [frames_in_pool, F], contiguous) is overwritten when given.  Shapes and dtypes are checked first; there is no CPU path."""
    _want(pool_features, "pool_features", torch.float32, (None, None))
    rows, F = pool_features.shape
    _want(offsets, "offsets", torch.int64, (None,))
    if offsets.numel() < 1:
        raise ValueError("ytvln.batch: `offsets` holds one entry per pool frame plus one")
    P = offsets.numel() - 1
    if out is not None:
        _want(out, "out", torch.float32, (P, F))
    tensors = [("pool_features", pool_features), ("offsets", offsets), ("out", out)]
    for name, t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"ytvln.batch: `{name}` must live on the GPU (no CPU path)")
    dev = pool_features.device
    if any(t is not None and t.device != dev for _, t in tensors):
        raise ValueError("ytvln.batch: global_rows needs all its tensors on one device")
    if out is None:
        out = torch.empty(P, F, dtype=torch.float32, device=dev)
    call("ytvln_pool_global_rows_f32", ops._ptr(pool_features), ops._ptr(offsets), P, rows, F, ops._ptr(out), ops._stream())
    return out


def expand_records(pool_features: Tensor, pool_geom: Tensor, pool_probs: Optional[Tensor], pool_global: Tensor, offsets: Tensor, index: Tensor,
                   boxes: int, view: Optional[Tensor] = None, out: Optional[Sequence[Optional[Tensor]]] = None, bad: Optional[Tensor] = None):
    """`expand_ragged` for a pool of RAW records (`ytvln_expand_records_f32`): the pool holds what comes off the disk, and what the
    reference's readers compute per frame on the host (`features_reader.py:91-124`, `:153-179`, `:258-341`) is done in the same launch:

        pool_features [rows, F] fp32   pool_probs [rows, C] fp32 or None   offsets [frames_in_pool + 1] int64   index [bs, K, frames] int64
        pool_geom   [rows, 8] fp32: x1, y1, x2, y2 in pixels, image width and height of the row's record, featureHeading, featureElevation
        pool_global [frames_in_pool, F] fp32: `global_rows(pool_features, offsets)`
        view        None, or fp64 [bs, K, frames, 2]: the agent's heading and next heading at each slot (the panorama reader's query)

    A slot showing a frame of n rows gets min(n + 1, boxes) real rows: the global region first (mean feature, whole-image box, uniform
    class distribution), then the frame's rows with their boxes normalised by the image size, the relative area in column 4 and, in
    columns 5-10, ones (`view` None) or the sines and cosines of featureHeading - heading, featureElevation and featureHeading - next
    heading.  Everything but those six columns equals the readers' output after `.float()` bit for bit; they are the fp64 functions of the
    fp32 angle rounded once.  The headings being a per-slot input, one viewpoint is one pool frame under whatever headings it is seen.

    Returns, `out` and `bad` as for `expand_ragged`; an EMPTY frame is a bad slot here (the readers raise for it).  Shapes and dtypes are
    checked first (ValueError, nothing touched); there is no CPU path."""
    boxes, rows, F, C, (bs, K, frames) = _check_pool(boxes, pool_features, [("pool_geom", pool_geom, 8)], pool_probs, offsets, index)
    _want(pool_global, "pool_global", torch.float32, (offsets.numel() - 1, F))
    if view is not None:
        _want(view, "view", torch.float64, (bs, K, frames, 2))
    if pool_probs is not None and C == 0:
        raise ValueError("ytvln.batch: `pool_probs` needs at least one class (the global region holds 1 / C)")
    f, bx, pr, m = _check_out("expand_records", [("pool_features", pool_features), ("pool_geom", pool_geom), ("pool_probs", pool_probs),
                                                 ("pool_global", pool_global), ("offsets", offsets), ("index", index), ("view", view)],
                              out, bad, (bs, K, frames * boxes), F, C)
    call("ytvln_expand_records_f32", ops._ptr(pool_features), ops._ptr(pool_geom), ops._ptr(pool_probs), ops._ptr(pool_global),
         ops._ptr(offsets), offsets.numel() - 1, rows, ops._ptr(index), ops._ptr(view), bs * K * frames, frames, boxes, F, C, ops._ptr(f),
         ops._ptr(bx), ops._ptr(pr), ops._ptr(m), ops._ptr(bad), ops._stream())
    return f, bx, pr, m


_FEATURE_DTYPES = {torch.float32: DT_F32, torch.bfloat16: DT_BF16}


def _check_masked(who: str, inputs, out, bad, lead, F: int, C: int, masked_vision: bool, p, feature_dtype):
    """`_check_out` for the masked expansions: `feature_dtype`, `p` and the five tensors of `out` (ValueError), then every tensor on the GPU
    (RuntimeError) and on one device.  Returns (image_features, image_boxes, image_targets, image_masks, image_targets_mask), allocated here
    when `out` is None; targets and targets mask are None when there are no `pool_probs` (masking off)."""
    if feature_dtype not in _FEATURE_DTYPES:
        raise ValueError(f"ytvln.batch: `feature_dtype` must be torch.float32 or torch.bfloat16, got {feature_dtype!r}")
    probs = dict(inputs)["pool_probs"] is not None
    if masked_vision and not probs:
        raise ValueError("ytvln.batch: masked_vision needs `pool_probs` (the targets of a selected region are its class probabilities)")
    if p is not None:
        if not masked_vision:
            raise ValueError("ytvln.batch: explicit draws `p` go with masked_vision=True")
        _want(p, "p", torch.float32, lead)
    if out is not None:
        if len(out) != 5:
            raise ValueError("ytvln.batch: `out` is (image_features, image_boxes, image_targets, image_masks, image_targets_mask)")
        f, bx, tg, m, tm = out
        _want(f, "out[0]", feature_dtype, (*lead, F))
        _want(bx, "out[1]", torch.float32, (*lead, 12))
        if (tg is None) == probs or (tm is None) == probs:
            raise ValueError("ytvln.batch: out[2] (image_targets), out[4] (image_targets_mask) and `pool_probs` go together: all given or all None")
        if tg is not None:
            _want(tg, "out[2]", torch.float32, (*lead, C))
            _want(tm, "out[4]", torch.int64, lead)
        _want(m, "out[3]", torch.int64, lead)
    if bad is not None:
        _want(bad, "bad", torch.int64, (1,))
    tensors = list(inputs) + [("p", p), ("bad", bad)] + ([(f"out[{i}]", t) for i, t in enumerate(out)] if out is not None else [])
    for name, t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"ytvln.batch: `{name}` must live on the GPU (no CPU path)")
    dev = inputs[0][1].device
    if any(t is not None and t.device != dev for _, t in tensors):
        raise ValueError(f"ytvln.batch: {who} needs all its tensors on one device")
    if out is None:
        f = torch.empty(*lead, F, dtype=feature_dtype, device=dev)
        bx = torch.empty(*lead, 12, dtype=torch.float32, device=dev)
        tg = torch.empty(*lead, C, dtype=torch.float32, device=dev) if probs else None
        m = torch.empty(*lead, dtype=torch.int64, device=dev)
        tm = torch.empty(*lead, dtype=torch.int64, device=dev) if probs else None
    return f, bx, tg, m, tm


def _draws(masked_vision: bool, p, device):
    """(p pointer, rng pointer, site, the DropoutState to keep alive) of a masked expansion: the explicit draws, or the next site of the
    device's Philox stream exactly as `randomize_regions` takes it, or nothing (masking off)."""
    if not masked_vision:
        return None, None, 0, None
    if p is not None:
        return ops._ptr(p), None, 0, None
    st = ops.DropoutState(device)
    return None, ops._ptr(st.tensor), st.next_site(), st


def expand_ragged_masked(pool_features: Tensor, pool_locations: Tensor, pool_probs: Optional[Tensor], offsets: Tensor, index: Tensor, boxes: int,
                         masked_vision: bool = True, p: Optional[Tensor] = None, feature_dtype=torch.float32,
                         out: Optional[Sequence[Optional[Tensor]]] = None, bad: Optional[Tensor] = None):
    """`expand_ragged` + `randomize_regions` (+ the bf16 rounding of the features the bf16-resident model applies) in ONE launch
    (`ytvln_expand_ragged_masked`): the MVM targets are written once, the features once in `feature_dtype` (torch.float32 or torch.bfloat16,
    each value rounded once to nearest even), and the padded class probabilities are never materialised.  Returns (image_features
    [bs, K, frames*boxes, F], image_boxes [.., 12], image_targets [.., C], image_masks [..] int64, image_targets_mask [..] int64): bit for bit
    what `expand_ragged` followed by `randomize_regions(features, probs, masks)` -- and `.to(torch.bfloat16)` -- gives, features in place
    included; drop them into entries 1, 2, 4, 3, 5 of the 16-tuple and call `mask_batch(..., vision_premasked=True)`.

    `p` (fp32 [bs, K, frames*boxes]) supplies the draws as it does for `randomize_regions`; without it the device's Philox stream
    (`ops.DropoutState`) supplies them exactly as for that function.  `masked_vision=False`: features unmasked, targets 1/C and a zero
    targets mask -- what `mask_batch(masked_vision=False)` returns; `pool_probs` may then be None, and targets and targets mask come back None
    (inference re-ranking: bf16 features, no probabilities).  `out` = the five tensors (the static inputs of a captured step; the two target
    entries None together with `pool_probs`); `bad` as for `expand_ragged`.  Shapes and dtypes are checked first (ValueError, nothing
    touched); there is no CPU path."""
    boxes, rows, F, C, (bs, K, frames) = _check_pool(boxes, pool_features, [("pool_locations", pool_locations, None)], pool_probs, offsets, index)
    L = pool_locations.shape[1]
    if L > 11:
        raise ValueError(f"ytvln.batch: `pool_locations` has {L} columns; the boxes hold 11 next to the position column")
    masked_vision = bool(masked_vision)
    f, bx, tg, m, tm = _check_masked("expand_ragged_masked", [("pool_features", pool_features), ("pool_locations", pool_locations),
                                                              ("pool_probs", pool_probs), ("offsets", offsets), ("index", index)],
                                     out, bad, (bs, K, frames * boxes), F, C, masked_vision, p, feature_dtype)
    p_ptr, rng_ptr, site, _keep = _draws(masked_vision, p, pool_features.device)
    call("ytvln_expand_ragged_masked", ops._ptr(pool_features), ops._ptr(pool_locations), ops._ptr(pool_probs), ops._ptr(offsets),
         offsets.numel() - 1, rows, ops._ptr(index), bs * K * frames, frames, boxes, F, L, C, p_ptr, rng_ptr, site, f.data_ptr(),
         _FEATURE_DTYPES[feature_dtype], ops._ptr(bx), ops._ptr(tg), ops._ptr(m), ops._ptr(tm), ops._ptr(bad), ops._stream())
    return f, bx, tg, m, tm


def expand_records_masked(pool_features: Tensor, pool_geom: Tensor, pool_probs: Optional[Tensor], pool_global: Tensor, offsets: Tensor,
                          index: Tensor, boxes: int, view: Optional[Tensor] = None, masked_vision: bool = True, p: Optional[Tensor] = None,
                          feature_dtype=torch.float32, out: Optional[Sequence[Optional[Tensor]]] = None, bad: Optional[Tensor] = None):
    """`expand_ragged_masked` for a pool of RAW records (`ytvln_expand_records_masked`): `expand_records` + `randomize_regions` (+ the bf16
    rounding) in one launch, same five outputs, same `masked_vision` / `p` / `feature_dtype` / `out` / `bad`.  The global region of a slot
    (row 0) is a region like any other: selected, its targets are its uniform distribution; zeroed, its feature row is zeros."""
    boxes, rows, F, C, (bs, K, frames) = _check_pool(boxes, pool_features, [("pool_geom", pool_geom, 8)], pool_probs, offsets, index)
    _want(pool_global, "pool_global", torch.float32, (offsets.numel() - 1, F))
    if view is not None:
        _want(view, "view", torch.float64, (bs, K, frames, 2))
    if pool_probs is not None and C == 0:
        raise ValueError("ytvln.batch: `pool_probs` needs at least one class (the global region holds 1 / C)")
    masked_vision = bool(masked_vision)
    f, bx, tg, m, tm = _check_masked("expand_records_masked", [("pool_features", pool_features), ("pool_geom", pool_geom),
                                                               ("pool_probs", pool_probs), ("pool_global", pool_global), ("offsets", offsets),
                                                               ("index", index), ("view", view)],
                                     out, bad, (bs, K, frames * boxes), F, C, masked_vision, p, feature_dtype)
    p_ptr, rng_ptr, site, _keep = _draws(masked_vision, p, pool_features.device)
    call("ytvln_expand_records_masked", ops._ptr(pool_features), ops._ptr(pool_geom), ops._ptr(pool_probs), ops._ptr(pool_global),
         ops._ptr(offsets), offsets.numel() - 1, rows, ops._ptr(index), ops._ptr(view), bs * K * frames, frames, boxes, F, C, p_ptr, rng_ptr, site,
         f.data_ptr(), _FEATURE_DTYPES[feature_dtype], ops._ptr(bx), ops._ptr(tg), ops._ptr(m), ops._ptr(tm), ops._ptr(bad), ops._stream())
    return f, bx, tg, m, tm


class _FramePool:
    """What RaggedPool and RecordPool share: per-row fp32 buffers `host_<name>` (pinned staging) / `<name>` (static device buffer) for every
    (name, columns) of `_columns`, `offsets`, `bad`, keys -> ids, `index`, `upload` and `reset`.  The subclasses say which arrays a frame
    consists of (`add`) and which kernels expand it (`expand`)."""

    def __init__(self, capacity_rows: int, capacity_frames: int, columns, device=None):
        kind = type(self).__name__
        capacity_rows, capacity_frames = int(capacity_rows), int(capacity_frames)
        if capacity_rows < 1 or capacity_frames < 1:
            raise ValueError(f"ytvln.batch: {kind} capacities must be positive, got {capacity_rows} rows, {capacity_frames} frames")
        self.capacity_rows, self.capacity_frames = capacity_rows, capacity_frames
        if device is None and torch.cuda.is_available():
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device) if device is not None else None
        if self.device is not None and self.device.type != "cuda":
            raise RuntimeError(f"ytvln.batch: {kind}'s device buffers must live on the GPU (no CPU path), got {self.device}")
        pin = self.device is not None
        self._columns = [(name, int(cols)) for name, cols in columns if cols is not None]
        for name, cols in columns:
            setattr(self, "host_" + name, torch.zeros(capacity_rows, int(cols), pin_memory=pin) if cols is not None else None)
            setattr(self, name, torch.zeros(capacity_rows, int(cols), device=self.device) if cols is not None and pin else None)
        self.host_offsets = torch.zeros(capacity_frames + 1, dtype=torch.int64, pin_memory=pin)
        self.offsets = self.bad = None
        if self.device is not None:
            self.offsets = torch.zeros(capacity_frames + 1, dtype=torch.int64, device=self.device)
            self.bad = torch.zeros(1, dtype=torch.int64, device=self.device)        # bad slots (see the expansion), summed over the calls
        self.rows = self.frames = 0
        self.bytes_uploaded = 0
        self._ids = {}
        self._uploaded = None

    @staticmethod
    def _rows_of(x, name: str, cols: int, n: int) -> Tensor:
        if torch.is_tensor(x):
            t = x
        else:
            with warnings.catch_warnings():         # decoded records are read-only views of the store's bytes; they are only read here
                warnings.simplefilter("ignore", UserWarning)
                t = torch.from_numpy(x)
        if t.dim() != 2 or t.shape[1] < cols or t.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"ytvln.batch: `{name}` must be an fp32 or fp64 array [n, {cols}], got {t.dtype} {list(t.shape)}")
        return t[:n, :cols]

    def _append(self, key, n: int, arrays) -> int:
        """Copy the first `n` rows of every (name, array) of one frame behind the rows in use and return the frame's id.  Nothing is written
        before every check has passed."""
        kind = type(self).__name__
        given = dict(arrays)
        if any((given.get(name) is None) != (getattr(self, "host_" + name) is None) for name in given):
            raise ValueError(f"ytvln.batch: this {kind} was built with probs={self.host_probs is not None}")
        cut = [(name, self._rows_of(given[name], name, cols, n)) for name, cols in self._columns]
        if any(t.shape[0] != n for _, t in cut):
            raise ValueError(f"ytvln.batch: {', '.join(name for name, _ in cut)} of a frame need the same number of rows (>= {n} here)")
        if self.frames + 1 > self.capacity_frames:
            raise ValueError(f"ytvln.batch: {kind} is full: capacity_frames = {self.capacity_frames}")
        if self.rows + n > self.capacity_rows:
            raise ValueError(f"ytvln.batch: {self.rows} + {n} rows exceed {kind}'s capacity_rows = {self.capacity_rows}")
        a, b = self.rows, self.rows + n
        for name, t in cut:
            getattr(self, "host_" + name)[a:b].copy_(t)            # fp64 -> fp32 by copy_: the rounding of `.float()`
        pid = self.frames
        self.frames, self.rows = pid + 1, b
        self.host_offsets[pid + 1] = b
        self._ids[key] = pid
        return pid

    @staticmethod
    def index(options, frames: int) -> Tensor:
        """int64 [bs, K, frames] from nested lists of pool ids (`options[item][option]` = the ids of that option's frames in order):
        cut to `frames` positions, padded with -1."""
        bs = len(options)
        K = max((len(o) for o in options), default=0)
        if any(len(o) != K for o in options):
            raise ValueError("ytvln.batch: every item needs the same number of options")
        idx = torch.full((bs, K, int(frames)), -1, dtype=torch.int64)
        for i, item in enumerate(options):
            for k, ids in enumerate(item):
                ids = list(ids)[:int(frames)]
                if ids:
                    idx[i, k, :len(ids)] = torch.as_tensor(ids, dtype=torch.int64)
        return idx

    def _need_device(self, what: str) -> None:
        if self.device is None:
            raise RuntimeError(f"ytvln.batch: {type(self).__name__}.{what} needs the GPU (no CPU path)")

    def upload(self) -> None:
        """Non-blocking copies of the used prefix of each buffer, and of `offsets`, to the device on the current stream.  Entries of
        `offsets` beyond the used frames repeat the last value: a stale index entry is an empty frame, not a wild read."""
        self._need_device("upload")
        self.host_offsets[self.frames + 1:] = self.rows
        moved = 0
        for name, _ in self._columns:
            d, h = getattr(self, name), getattr(self, "host_" + name)
            if self.rows:
                d[:self.rows].copy_(h[:self.rows], non_blocking=True)
            moved += self.rows * h.shape[1] * h.element_size()
        self.offsets.copy_(self.host_offsets, non_blocking=True)
        moved += self.host_offsets.numel() * self.host_offsets.element_size()
        self.bytes_uploaded = moved
        self._uploaded = torch.cuda.Event()
        self._uploaded.record()

    def reset(self) -> None:
        """Start the next step: forget the frames and keys (the buffers stay)."""
        if self._uploaded is not None:
            self._uploaded.synchronize()           # the staging buffers are about to be overwritten
            self._uploaded = None
        self.rows = self.frames = 0
        self._ids = {}


class RaggedPool(_FramePool):
    """The frames of one step as the feature readers return them, shipped once: pinned host staging buffers and static device buffers of
    fixed capacity, allocated here and reused every step.

        pool = RaggedPool(capacity_rows, capacity_frames)
        ids  = [pool.add(key, *reader[key], max_rows=boxes) for key in ...]      # one frame each; a key seen before costs nothing
        idx  = pool.index(options, frames)                                         # nested lists of ids -> int64 [bs, K, frames]
        pool.upload()                                                              # the used rows only, non-blocking, current stream
        f, bx, pr, m = pool.expand(idx, boxes, out=static_inputs)                  # one launch (expand_ragged)
        pool.reset()                                                               # next step

    `add` converts fp64 arrays (the readers' locations and probabilities) to fp32 exactly as the reference's `.float()` does.  The device
    buffers never move, so a captured `expand` replays on whatever the last `upload()` brought.  `reset()` waits for the last upload's
    copies before the staging buffers are written again.  Without a GPU the object still does its host bookkeeping (tests); `upload` and
    `expand` then raise."""

    def __init__(self, capacity_rows: int, capacity_frames: int, feature_dim: int = 2048, loc_dim: int = 11, num_classes: int = 1601,
                 device=None, probs: bool = True):
        if not 0 <= int(loc_dim) <= 11:
            raise ValueError(f"ytvln.batch: loc_dim must be within [0, 11], got {loc_dim}")
        self.feature_dim, self.loc_dim, self.num_classes = int(feature_dim), int(loc_dim), int(num_classes)
        super().__init__(capacity_rows, capacity_frames, [("features", self.feature_dim), ("locations", self.loc_dim),
                                                          ("probs", self.num_classes if probs else None)], device)

    def add(self, key, features, locations, probs=None, max_rows: Optional[int] = None) -> int:
        """Append one frame (the tuple a reader's `__getitem__` returns) and return its pool id.  A key seen since the last `reset()`
        returns its id and copies nothing.  `max_rows` keeps the first rows only (`num_boxes = min(len, max_num_boxes)`)."""
        known = self._ids.get(key)
        if known is not None:
            return known
        n = int(features.shape[0])
        if max_rows is not None:
            n = min(n, int(max_rows))
        return self._append(key, n, [("features", features), ("locations", locations), ("probs", probs)])

    def expand(self, index: Tensor, boxes: int, out=None):
        """`expand_ragged` on the device buffers (a CPU `index` is uploaded first)."""
        self._need_device("expand")
        if torch.is_tensor(index) and not index.is_cuda:
            index = index.to(self.device, non_blocking=True)
        return expand_ragged(self.features, self.locations, self.probs, self.offsets, index, boxes, out=out, bad=self.bad)

    def expand_masked(self, index: Tensor, boxes: int, masked_vision: bool = True, feature_dtype=torch.float32, out=None):
        """`expand_ragged_masked` on the device buffers (a CPU `index` is uploaded first): `expand` with the region masking, and the bf16
        rounding of the features when asked for, in the same launch.  The draws are the device's Philox stream's."""
        self._need_device("expand_masked")
        if torch.is_tensor(index) and not index.is_cuda:
            index = index.to(self.device, non_blocking=True)
        return expand_ragged_masked(self.features, self.locations, self.probs, self.offsets, index, boxes, masked_vision=masked_vision,
                                    feature_dtype=feature_dtype, out=out, bad=self.bad)


class RecordPool(_FramePool):
    """RaggedPool for RAW records: the frames of one step as they come off the disk (`reader.records(query)` / `reader.record(key)`:
    features, geometry, probabilities, all fp32), shipped once; the global region, the box normalisation and the orientation columns are
    computed on the device (`global_rows` + `expand_records`), so the host only decodes.

        pool = RecordPool(capacity_rows, capacity_frames)
        ids  = [pool.add(key, *reader.records(key)) for key in ...]                # ALL rows of the frame: the mean runs over every region
        idx  = pool.index(options, frames)
        pool.upload()
        f, bx, pr, m = pool.expand(idx, boxes, view=headings, out=static_inputs)   # two launches on the current stream
        pool.reset()

    A panorama viewpoint is one frame whatever headings it is seen under: the headings are `view` (fp64 [bs, K, frames, 2]), not part of
    the key.  The device buffers never move, so a captured `expand` replays on whatever the last `upload()` brought (and on whatever the
    static `index` / `view` tensors hold).  Lifecycle, `bad` and the behaviour without a GPU are RaggedPool's."""

    def __init__(self, capacity_rows: int, capacity_frames: int, feature_dim: int = 2048, num_classes: int = 1601, device=None,
                 probs: bool = True):
        self.feature_dim, self.num_classes = int(feature_dim), int(num_classes)
        super().__init__(capacity_rows, capacity_frames, [("features", self.feature_dim), ("geom", 8),
                                                          ("probs", self.num_classes if probs else None)], device)
        self.global_features = None                 # [capacity_frames, F]: written by every expand() ahead of the expansion
        if self.device is not None:
            self.global_features = torch.zeros(self.capacity_frames, self.feature_dim, device=self.device)

    def add(self, key, features, geom, probs=None) -> int:
        """Append one frame -- every row of it: the reference's mean runs over all regions, also over those the expansion cuts -- and
        return its pool id.  A key seen since the last `reset()` returns its id and copies nothing.  An empty frame is an error, as it
        is for the readers ("Features could not be correctly read")."""
        known = self._ids.get(key)
        if known is not None:
            return known
        n = int(features.shape[0])
        if n < 1:
            raise ValueError(f"ytvln.batch: frame {key!r} is empty: features could not be correctly read")
        return self._append(key, n, [("features", features), ("geom", geom), ("probs", probs)])

    def expand(self, index: Tensor, boxes: int, view: Optional[Tensor] = None, out=None):
        """`global_rows` + `expand_records` on the device buffers (a CPU `index` or `view` is uploaded first)."""
        self._need_device("expand")
        if torch.is_tensor(index) and not index.is_cuda:
            index = index.to(self.device, non_blocking=True)
        if torch.is_tensor(view) and not view.is_cuda:
            view = view.to(self.device, non_blocking=True)
        global_rows(self.features, self.offsets, out=self.global_features)
        return expand_records(self.features, self.geom, self.probs, self.global_features, self.offsets, index, boxes, view=view, out=out,
                              bad=self.bad)

    def expand_masked(self, index: Tensor, boxes: int, view: Optional[Tensor] = None, masked_vision: bool = True, feature_dtype=torch.float32,
                      out=None):
        """`global_rows` + `expand_records_masked` on the device buffers (a CPU `index` or `view` is uploaded first): `expand` with the region
        masking, and the bf16 rounding of the features when asked for, in the expansion's launch."""
        self._need_device("expand_masked")
        if torch.is_tensor(index) and not index.is_cuda:
            index = index.to(self.device, non_blocking=True)
        if torch.is_tensor(view) and not view.is_cuda:
            view = view.to(self.device, non_blocking=True)
        global_rows(self.features, self.offsets, out=self.global_features)
        return expand_records_masked(self.features, self.geom, self.probs, self.global_features, self.offsets, index, boxes, view=view,
                                     masked_vision=masked_vision, feature_dtype=feature_dtype, out=out, bad=self.bad)


def mask_batch(batch: Sequence[Tensor], vocab_size: int = VOCAB_SIZE, mask_token_id: int = MASK_TOKEN_ID, masked_language: bool = True,
               masked_vision: bool = True, mask_action_rate: float = 0.0, args=None, vision_premasked: bool = False) -> List[Tensor]:
    """Apply both maskings to an un-masked device batch in the 16-tuple layout of `get_model_input` (utils/utils_init.py:34-53):
    1 image_features, 3 image_masks, 4 image_targets (class probabilities in, MVM targets out), 5 image_targets_mask (out),
    6 instr_tokens [bs, K, T], 7 instr_mask, 8 instr_targets (out).

    `masked_language` / `masked_vision` / `mask_action_rate` are the reference's options of the same names; `args` (the parsed command
    line) supplies all three when given.  A disabled masking returns what the reference's dataset returns (`all_dataset.py:251-261`):
    instr_targets = -1, or image_targets = 1/C with a zero image_targets_mask, and the inputs untouched.  The action draw is per
    dataset item, i.e. per row of the batch dimension: all K instructions of an item together, like the reference.

    `vision_premasked=True`: entries 1, 4 and 5 already are what the vision masking produces (a pool's `expand_masked` wrote them) and are
    left exactly as they came, whatever `masked_vision` says; the token side works as before."""
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
    if vision_premasked:
        pass                            # entries 1, 4, 5 stay the objects the pool's expand_masked wrote
    elif masked_vision:
        b[1], b[4], b[5] = randomize_regions(b[1], b[4], b[3])
    else:
        b[4], b[5] = torch.ones_like(b[4]) / b[4].shape[-1], torch.zeros_like(b[3])
    return b
