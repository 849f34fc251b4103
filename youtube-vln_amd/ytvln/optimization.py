"""Fused AdamW + LR schedules with the reference's semantics (`vilbert/optimization.py`).

`AdamW` keeps the reference constructor (`AdamW(params, lr, betas, eps, weight_decay, correct_bias)`), the per-parameter
state layout (`step`, `exp_avg`, `exp_avg_sq` -> checkpoints stay interchangeable) and its exact update rule
(`optimization.py:141-187`: denom = sqrt(v)+eps, bias correction folded into the step size, decoupled decay applied AFTER
the update, tensors without a gradient skipped entirely).  Execution differs: on the first `step()` the parameters that
received a gradient are moved into one flat fp32 arena (their `.data` / `.grad` become views), moments live in two more
arenas, and a whole step is one HIP kernel launch per (param-group, step-count) class instead of ~8 ATen kernels per
tensor x 541 tensors.  The flat gradient arena is also what the data-parallel all-reduce buckets (ytvln/distributed.py).

Beyond the reference, as plain attributes (the `AdamW` docstring): `max_grad_norm` / `skip_nonfinite` bound the global gradient norm inside
the step, `trust_ratio` switches the update to LAMB's layer-wise trust ratio, `ema_decay` keeps an exponential moving average of the weights
in a shadow arena, `tensor_stats` reports norms, maxima and non-finite counts per parameter tensor.
"""
from __future__ import annotations

import contextlib
import math
import numbers
import struct
from collections import OrderedDict
from typing import Dict, List, NamedTuple, Optional

import torch
from torch.optim import Optimizer
from torch.optim.lr_scheduler import LambdaLR

from . import ops


CHUNK = 16384       # elements per workgroup of the fused kernel
ALIGN = 4           # arena offsets are multiples of 4 floats (16-byte vector access)


def lamb_tables(tensors, chunk=CHUNK):
    """The two int32 tables of the LAMB launches for one chunk table built from `tensors` = [(index in the arena, numel)] in table order
    (every tensor cut into records of `chunk` elements, contiguous): (tensor_first: the first record of each tensor, len(tensors) + 1
    entries; rec_tensor: the arena index of every record's tensor)."""
    first, rec = [0], []
    for k, numel in tensors:
        if numel <= 0 or k < 0:
            raise ValueError(f"lamb_tables: tensor {k} with {numel} elements")
        rec += [int(k)] * ((numel + chunk - 1) // chunk)
        first.append(len(rec))
    return first, rec


def chunk_table(runs, chunk=CHUNK):
    """(bytearray, number of records): the chunk table of `runs` = [(arena offset, numel, weight decay)], every run cut into records
    (offset, length, weight decay, 0) of at most `chunk` elements."""
    rec, n = bytearray(), 0
    for o, numel, wd in runs:
        for c in range(0, numel, chunk):
            rec += struct.pack("<qqff", o + c, min(chunk, numel - c), wd, 0.0)
            n += 1
    return rec, n


def new_arena(flat, index, ids):
    """The arena record: the flat fp32 tensors p, g, m, v of `flat`, index = {id(param): (offset, numel)}, ids = the members in order, and
    every lazily created buffer still absent: the bf16 weight copy (pb, pb_versions), the bf16 exchange buffer (gb) and the buffers of the
    opt-in features (partials and clip; lamb; ema; stats)."""
    return dict(flat, index=index, ids=ids, pb=None, pb_versions={}, gb=None, partials=None, clip=None, lamb=None, ema=None, stats=None)


class CaptureSettings(NamedTuple):
    """What a captured step bakes in (AdamW.capture_settings()): each field changes which launches a step records."""
    clip: Optional[tuple] = None        # None or (max_norm, skip_nonfinite)
    lamb: bool = False
    ema: bool = False                   # on / off only: decay and warm-up travel by value
    stats: bool = False


_SETTING_ATTRS = {"clip": "max_grad_norm / skip_nonfinite", "lamb": "trust_ratio", "ema": "ema_decay (on / off)", "stats": "tensor_stats"}


class ConstantLRSchedule(LambdaLR):
    """optimization.py:26-30."""

    def __init__(self, optimizer, last_epoch=-1):
        super().__init__(optimizer, lambda _: 1.0, last_epoch=last_epoch)


class WarmupConstantSchedule(LambdaLR):
    """optimization.py:33-45."""

    def __init__(self, optimizer, warmup_steps, last_epoch=-1):
        self.warmup_steps = warmup_steps
        super().__init__(optimizer, self.lr_lambda, last_epoch=last_epoch)

    def lr_lambda(self, step):
        if step < self.warmup_steps:
            return float(step) / float(max(1.0, self.warmup_steps))
        return 1.0


class WarmupLinearSchedule(LambdaLR):
    """optimization.py:48-61: linear warm-up to 1 over `warmup_steps`, then linear decay to 0 at `t_total`."""

    def __init__(self, optimizer, warmup_steps, t_total, last_epoch=-1):
        self.warmup_steps = warmup_steps
        self.t_total = t_total
        super().__init__(optimizer, self.lr_lambda, last_epoch=last_epoch)

    def lr_lambda(self, step):
        if step < self.warmup_steps:
            return float(step) / float(max(1, self.warmup_steps))
        return max(0.0, float(self.t_total - step) / float(max(1.0, self.t_total - self.warmup_steps)))


class WarmupCosineSchedule(LambdaLR):
    """optimization.py:64-82: linear warm-up, then 0.5 * (1 + cos(2 pi cycles progress)) over the remaining steps (half a period by default),
    floored at 0."""

    def __init__(self, optimizer, warmup_steps, t_total, cycles=0.5, last_epoch=-1):
        self.warmup_steps, self.t_total, self.cycles = warmup_steps, t_total, cycles
        super().__init__(optimizer, self.lr_lambda, last_epoch=last_epoch)

    def lr_lambda(self, step):
        if step < self.warmup_steps:
            return float(step) / float(max(1.0, self.warmup_steps))
        progress = float(step - self.warmup_steps) / float(max(1, self.t_total - self.warmup_steps))
        return max(0.0, 0.5 * (1.0 + math.cos(2.0 * math.pi * float(self.cycles) * progress)))


class WarmupCosineWithHardRestartsSchedule(LambdaLR):
    """optimization.py:85-105: linear warm-up, then `cycles` cosine decays from 1 to 0 with hard restarts; 0 once the schedule is over."""

    def __init__(self, optimizer, warmup_steps, t_total, cycles=1.0, last_epoch=-1):
        self.warmup_steps, self.t_total, self.cycles = warmup_steps, t_total, cycles
        super().__init__(optimizer, self.lr_lambda, last_epoch=last_epoch)

    def lr_lambda(self, step):
        if step < self.warmup_steps:
            return float(step) / float(max(1, self.warmup_steps))
        progress = float(step - self.warmup_steps) / float(max(1, self.t_total - self.warmup_steps))
        if progress >= 1.0:
            return 0.0
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * ((float(self.cycles) * progress) % 1.0))))


class AdamW(Optimizer):
    """The reference's AdamW, fused (module docstring), plus four opt-in features the reference does not have.

    What holds for every opt-in attribute below: it is a plain attribute -- not a constructor argument, not in `param_groups` / `defaults`,
    not in `state_dict()` (checkpoints stay interchangeable with the reference) -- and is validated when the step is taken: an invalid value
    raises a ValueError that names it, before anything is exchanged, launched or recorded.  Off (the default), a step launches and allocates
    exactly what it always did.  On, every step -- eager, while capturing, on replay -- runs the feature's launches: no host
    synchronisation, no atomics, fixed summation orders.  A captured step bakes the settings in (`capture_settings()`): changing one
    afterwards makes the next `prepare_replay()` raise; capture the step again.  Capturing with a feature on needs its device buffers, which
    must not live in a graph's pool: the first eager step with it on allocates them, or `capture_buffers()`, or the feature's own accessor.
    They are dropped with the arena (load_state_dict, a changed parameter set) -- the counts kept in them restart -- and are never part of
    `state_dict()`.

    max_grad_norm (default None): a number > 0 bounds the global L2 norm of the gradient the update applies -- after the data-parallel
        exchange and its 1/world average, over the bf16 sums when the exchange is bf16 -- with torch.nn.utils.clip_grad_norm_'s formula,
        coef = min(1, max_norm / (norm + 1e-6)); float("inf") measures the norm without clipping.  Anything else (<= 0, NaN, not a
        number) is invalid.
    skip_nonfinite (default False): a step whose gradient norm is inf or NaN leaves parameters, moments and the bf16 weight copy untouched
        and is counted.  Without it a non-finite norm behaves as in torch (error_if_nonfinite=False): the coefficient becomes 0 or NaN and
        goes into the update.
    With either set, a step runs, between the gradient exchange and the update: ytvln_grad_sumsq over every launch class, one
    ytvln_grad_clip_coef, then ytvln_adamw_clip per class.  The decision to skip is taken on the device: the host cannot know it without a
    sync, so on a skipped step `state[p]["step"]` (the bias-correction count) and an LR scheduler still advance.  `grad_norm()` is a 0-d
    device view of the last step's norm (no sync); `skipped_steps()` reads the count of skipped steps back (synchronises).  Both settings
    are baked into a capture; the two small buffers are `clip_buffers()`.

    trust_ratio (default False; anything but a bool is invalid): True turns the update into LAMB (You et al., 2020) -- the AdamW direction
        with the decay inside it, r = b * m / (sqrt(v) + eps) + wd * p (b: the bias correction), rescaled per parameter tensor:
        p -= lr * trust * r with trust = ||p|| / ||r|| over the whole tensor.  Tensors of a group without weight decay (bias, LayerNorm:
        the BERT LAMB recipe) and tensors with a zero or non-finite norm keep trust = 1.  The gradient is the one plain AdamW would read
        (after the exchange, times grad_scale, times the clip coefficient with clipping on: LAMB's usual pre-normalisation IS
        max_grad_norm = 1).  Per launch class three launches replace the one update: ytvln_lamb_stage1 (moments and per-record partial
        norms), ytvln_lamb_trust, ytvln_lamb_stage2 (the update, and the bf16 weight copy): 40 bytes per parameter against 28.  With False
        the decay stays after the update.  Buffers: `lamb_buffers()`.  `trust_ratios()` is a device view [tensors in arena order, 4] of the
        last step's rows [||p||, ||r||, trust, 0].

    ema_decay (default None; a bool, a NaN or a value outside (0, 1) is invalid): a number strictly inside (0, 1) keeps an exponential
        moving average of the weights (timm's ModelEmaV2) in a shadow arena with the offsets of the parameter arena: the shadow starts as a
        copy of the weights, and behind the update launches of every chunk table one ytvln_ema_update applies e = fma(w, p - e, e) in fp32
        to the parameters the update just wrote (12 bytes per parameter, a launch of its own).  w = float32(1 - decay_eff) is computed on
        the host in double and travels through slot 6 of the per-class hyper record, so `ema_decay` and `ema_warmup` may change between
        replays of a captured step: only on / off is baked into a capture.
    ema_warmup (default False; anything but a bool is invalid): True gives decay_eff = min(ema_decay, (1 + n) / (10 + n)), n = `ema_updates`.
    ema_updates: the host count n of EMA updates taken.  Like `state[p]["step"]` it advances on a step the device decides to skip
        (skip_nonfinite): the host cannot know the decision without a sync; the shadow itself is left untouched by such a step.
    The shadow (`ema_buffers()`) is the one buffer that survives an arena rebuild: members that had a shadow keep it, new members start from
    their current value; parameters that never receive a gradient have none -- their EMA is the parameter itself.  Every data-parallel rank
    computes the same shadow: nothing is exchanged.  `ema_parameters()` maps parameters to their shadow views, `ema_state_dict(model)` is the
    model file with the shadow weights, `swap_ema()` / `with optimizer.ema_weights():` exchange weights and shadow in place for evaluation
    (views, arena slots and captured graphs stay valid; stepping while swapped raises RuntimeError), `ema_checkpoint(model)` /
    `load_ema(state, model)` carry the shadow through checkpoints (ytvln.utils_init.save_model, ytvln.vilbert_init.restore_checkpoint).

    tensor_stats (default False; anything but a bool is invalid): True makes every step report per parameter tensor what the step did:
        behind the update launches (and the EMA launch) of the step, ytvln_tensor_stats_stage1 and ytvln_tensor_stats_stage2 run over every
        launch class's whole chunk table (8 bytes per parameter read, 6 with bf16 gradients).  `tensor_stats_report()` returns two device
        views in arena order: rows [||g||, max |g|, ||p||, max |p|] over the finite elements and rows [non-finite elements of g, of p,
        steps so far with a non-finite g]; g is the gradient the update read (after the exchange, the bf16 sums with the bf16 exchange,
        times grad_scale, unclipped -- the quantity grad_norm() describes), p the parameter the next forward will use.  A step the device
        skipped (skip_nonfinite) leaves p unchanged and still reports: `nonfinite_tensors(model)` names the tensors whose gradient went
        non-finite (it synchronises), `tensor_names(model)` the rows.  Buffers: `stats_buffers()`; the sticky third count goes with them."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, correct_bias=True):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {} - should be >= 0.0".format(lr))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[1]))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {} - should be >= 0.0".format(eps))
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, correct_bias=correct_bias))
        self._arena = None          # dict(p, g, m, v flat tensors; index: id(param) -> (offset, numel))
        self._launch = None         # list of launch classes
        self.grad_scale = 1.0       # multiplied into the gradient inside the kernel (set by data-parallel wrappers)
        # torch.bfloat16 (set by data-parallel wrappers with the bf16 exchange): the update reads the bf16 exchange buffer (grad_bf16()),
        # not the fp32 arena.  Local accumulation stays fp32 either way.
        self.exchange_dtype = torch.float32
        # the opt-in features (class docstring): plain attributes, never part of state_dict()
        self.max_grad_norm = None   # global gradient-norm clipping
        self.skip_nonfinite = False
        self.trust_ratio = False    # LAMB layer-wise trust ratio
        self.ema_decay = None       # EMA of the weights
        self.ema_warmup = False
        self.ema_updates = 0        # EMA updates taken (host count; advances on a device-skipped step as state[p]["step"] does)
        self.tensor_stats = False   # per-tensor gradient / weight statistics
        self._captured = None       # the CaptureSettings recorded into the last captured step (None: nothing captured yet)
        self._group_slot = 0        # group_update(): the next free slot of the clip partials in this step
        self._ema_swapped = False   # swap_ema(): the parameter arena currently holds the shadow weights
        self._ema_carry = {}        # id(param) -> shadow values waiting for the next arena (rebuild, load_ema)

    # ---- arena management -----------------------------------------------------------------------------------------
    def _members(self):
        return [(gi, p) for gi, g in enumerate(self.param_groups) for p in g["params"] if p.grad is not None]

    def arena_layout(self) -> Dict[int, tuple]:
        return {} if self._arena is None else dict(self._arena["index"])

    def _build_arena(self, members):
        dev = members[0][1].device
        for _, p in members:
            if p.dtype != torch.float32 or not p.is_cuda:
                raise RuntimeError("ytvln AdamW needs fp32 parameters on a HIP device (no CPU fallback)")
            if p.grad.is_sparse:
                raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
        old = self._arena
        index, off = {}, 0
        for _, p in members:
            index[id(p)] = (off, p.numel())
            off += (p.numel() + ALIGN - 1) // ALIGN * ALIGN
        flat = {k: torch.zeros(off, dtype=torch.float32, device=dev) for k in ("p", "g", "m", "v")}
        with torch.no_grad():
            for _, p in members:
                o, n = index[id(p)]
                flat["p"][o:o + n].copy_(p.data.reshape(-1))
                flat["g"][o:o + n].copy_(p.grad.reshape(-1))
                st = self.state[p]
                if "exp_avg" in st:                      # carried over from a previous arena / a loaded checkpoint
                    flat["m"][o:o + n].copy_(st["exp_avg"].reshape(-1))
                    flat["v"][o:o + n].copy_(st["exp_avg_sq"].reshape(-1))
                else:
                    st["step"] = 0
                p.data = flat["p"][o:o + n].view(p.shape)
                p.grad = flat["g"][o:o + n].view(p.shape)
                st["exp_avg"] = flat["m"][o:o + n].view(p.shape)
                st["exp_avg_sq"] = flat["v"][o:o + n].view(p.shape)
        self._stash_ema(old)
        self._arena = new_arena(flat, index, [id(p) for _, p in members])
        self._launch = None
        del old
        if self._ema_carry and self.ema_decay is not None and not torch.cuda.is_current_stream_capturing():
            self.ema_buffers()      # a shadow existed (or was loaded) and the feature is on: it moves into the new arena at once
        # let the weight-gradient GEMMs write straight into the gradient arena and the packed projections alias the
        # parameter arena: every member parameter carries its slot (ytvln.ops.ArenaSlot)
        self._written = set()
        import weakref
        me = weakref.ref(self)
        for _, p in members:
            o, n = index[id(p)]
            p._ytvln_slot = ops.ArenaSlot(flat["p"], flat["g"], o, n, self._written, me)

    def bf16_arena(self, params=None):
        """The bf16 copy of the parameter arena (bf16-resident path, ytvln.ops._bf16_weight): created on first use by one cast of the whole
        arena, from then on refreshed by the AdamW kernel itself (ytvln_adamw_f32_bf16copy).  `params`: the parameters about to be read --
        if torch modified one of them in place since the copy was made (load_state_dict, manual edits: their version counters moved), its
        slice is cast again.  None before the arena exists."""
        a = self._arena
        if a is None:
            return None
        if a["pb"] is None:
            with ops.TwoStream.shared_write():
                a["pb"] = torch.empty(a["p"].numel(), dtype=torch.bfloat16, device=a["p"].device)
                ops.call("ytvln_cast_f32_bf16", a["p"].data_ptr(), a["p"].numel(), 1, a["p"].numel(), a["pb"].data_ptr(), a["p"].numel(), ops._stream())
            a["pb_versions"] = {id(p): p._version for _, p in self._members()}
        vers = a["pb_versions"]
        for p in (params or ()):
            rng = a["index"].get(id(p))
            if rng is None:
                return None
            if vers.get(id(p)) != p._version:
                if id(p) in vers:          # modified behind the optimizer's back: refresh this slice
                    o, n = rng
                    with ops.TwoStream.shared_write():
                        ops.call("ytvln_cast_f32_bf16", a["p"].data_ptr() + 4 * o, n, 1, n, a["pb"].data_ptr() + 2 * o, n, ops._stream())
                vers[id(p)] = p._version
        return a["pb"]

    def grad_bf16(self):
        """The send / receive buffer of the bf16 gradient exchange: bf16, the size and offsets of the fp32 gradient arena, allocated on first
        use (zeros: the padding between slots stays zero) and dropped with the arena.  Not part of state_dict.  None before the arena
        exists."""
        a = self._arena
        if a is None:
            return None
        if a["gb"] is None:
            with ops.TwoStream.shared_write():
                a["gb"] = torch.zeros(a["g"].numel(), dtype=torch.bfloat16, device=a["g"].device)
        return a["gb"]

    def pack_grads(self, tables=None):
        """Round the fp32 gradients to bf16 into grad_bf16(), on the current stream: over the chunk tables of every launch class (None) or
        over `tables` = [(launch class index, chunk table, number of chunks)] (one group of group_tables())."""
        gb = self.grad_bf16()
        if tables is None:
            tables = [(ci, c["table"], c["n"]) for ci, c in enumerate(self._launch)]
        for _, table, n in tables:
            ops.grad_pack_bf16(self._arena["g"], gb, table, n)

    # ---- what the opt-in features share ------------------------------------------------------------------------------
    def capture_settings(self) -> CaptureSettings:
        """The validated settings a captured step bakes in.  Raises ValueError for any invalid opt-in attribute."""
        return CaptureSettings(self.clip_settings(), self.lamb_setting(), self.ema_setting() is not None, self.stats_setting())

    def _arena_records(self) -> int:
        """CHUNK records of the whole arena: what the per-record partials of the features are sized by."""
        return sum((numel + CHUNK - 1) // CHUNK for _, numel in self._arena["index"].values())

    def _feature_buffers(self, key, attr, accessor, alloc):
        """The buffers `_arena[key]` of an opt-in feature, the one rule for all of them: None before the arena exists; allocated on first
        use by `alloc(arena, device)` -- callers ask only with the feature on, and never while capturing, where the buffers would live in
        the graph's pool --; dropped with the arena; not part of state_dict."""
        a = self._arena
        if a is None:
            return None
        if a[key] is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{attr} was switched on after the last eager step: take one eager step with it on (or call "
                                   f"{accessor}()) before capturing, so that its buffers do not live in a graph's pool")
            a[key] = alloc(a, a["g"].device)
        return a[key]

    def capture_buffers(self):
        """Allocate now, eagerly, whatever the current settings need, so that nothing of it lives in a graph's pool: the bf16 exchange
        buffer and the buffers of every feature that is on."""
        now = self.capture_settings()
        if self.exchange_dtype == torch.bfloat16:
            self.grad_bf16()
        for on, buffers in ((now.clip is not None, self.clip_buffers), (now.lamb, self.lamb_buffers), (now.ema, self.ema_buffers),
                            (now.stats, self.stats_buffers)):
            if on:
                buffers()

    # ---- global gradient-norm clipping ------------------------------------------------------------------------------
    def clip_settings(self):
        """None with the feature off, else (max_norm as a float -- inf: measure only --, skip_nonfinite).  Raises ValueError for a
        max_grad_norm that is not a number > 0."""
        mx = self.max_grad_norm
        if mx is None and not self.skip_nonfinite:
            return None
        if mx is None:
            return math.inf, True
        if isinstance(mx, bool) or not isinstance(mx, numbers.Real):
            raise ValueError(f"max_grad_norm must be None or a number > 0, got {mx!r}")
        mx = float(mx)
        if not mx > 0.0:          # (also a NaN)
            raise ValueError(f"max_grad_norm must be > 0, got {mx!r}")
        return mx, bool(self.skip_nonfinite)

    def clip_buffers(self):
        """(partials, clip): one fp32 partial per CHUNK record of the arena and the record [norm, coef, skip, skipped steps] the kernels
        exchange (_feature_buffers: None before the arena exists)."""
        def alloc(a, dev):
            a["partials"] = torch.zeros(self._arena_records(), dtype=torch.float32, device=dev)
            return torch.zeros(4, dtype=torch.float32, device=dev)
        clip = self._feature_buffers("clip", "max_grad_norm / skip_nonfinite", "clip_buffers", alloc)
        return None if clip is None else (self._arena["partials"], clip)

    def _clip_record(self):
        """The clip record when clipping is on, else None: what the clip-aware launches take."""
        return self.clip_buffers()[1] if self.clip_settings() is not None else None

    def _grad_operand(self):
        """The gradient the update reads: the fp32 arena, or the bf16 sums of the bf16 exchange."""
        a = self._arena
        if self.exchange_dtype == torch.bfloat16:
            if a["gb"] is None:
                raise RuntimeError("bf16 gradient exchange: the update would read a bf16 buffer nothing was packed into")
            return a["gb"]
        return a["g"]

    def sumsq_tables(self, tables, slot):
        """ytvln_grad_sumsq over `tables` = [(launch class index, chunk table, number of chunks)] on the current stream, into the partials
        from `slot` on; returns the next free slot."""
        partials, _ = self.clip_buffers()
        g = self._grad_operand()
        for _, table, n in tables:
            if slot + n > partials.numel():
                raise RuntimeError("gradient clipping: more chunk records than the arena has")
            ops.grad_sumsq(g, table, n, partials[slot:slot + n])
            slot += n
        return slot

    def clip_coef(self, n):
        """ytvln_grad_clip_coef over the first `n` partials on the current stream: from here on the clip record is this step's."""
        max_norm, skip = self.clip_settings()
        partials, clip = self.clip_buffers()
        ops.grad_clip_coef(partials, n, self.grad_scale, max_norm, skip, clip)

    def grad_norm(self):
        """0-d device tensor: the global L2 norm of the gradient the last step applied (before clipping, after the 1/world average).  A
        view of the clip record -- no synchronisation; later steps overwrite it."""
        a = self._arena
        if a is None or a["clip"] is None:
            raise RuntimeError("grad_norm(): no step has been taken with max_grad_norm / skip_nonfinite set")
        return a["clip"][0]

    def skipped_steps(self) -> int:
        """Steps skipped for a non-finite gradient norm since the arenas were built.  Reads a device counter: SYNCHRONISES."""
        a = self._arena
        if a is None or a["clip"] is None:
            return 0
        return int(a["clip"][3].item())

    # ---- LAMB layer-wise trust ratio ----------------------------------------------------------------------------------
    def lamb_setting(self) -> bool:
        """trust_ratio, validated: anything but a bool raises ValueError."""
        if not isinstance(self.trust_ratio, bool):
            raise ValueError(f"trust_ratio must be True or False, got {self.trust_ratio!r}")
        return self.trust_ratio

    def lamb_buffers(self):
        """(partials, trust, report): two fp32 partials per CHUNK record of the arena, one trust ratio and one report row
        [||p||, ||r||, trust, 0] per arena tensor (_feature_buffers: None before the arena exists)."""
        def alloc(a, dev):
            n, nt = self._arena_records(), len(a["index"])
            a["lamb_stepped"] = False
            return (torch.zeros(2 * n, dtype=torch.float32, device=dev), torch.ones(nt, dtype=torch.float32, device=dev),
                    torch.zeros(nt, 4, dtype=torch.float32, device=dev))
        return self._feature_buffers("lamb", "trust_ratio", "lamb_buffers", alloc)

    def trust_ratios(self):
        """Device tensor [tensors in arena order (arena_layout()), 4]: the rows [||p||, ||r||, trust, 0] of the last LAMB step, the norms
        being those of the pre-update parameter and of the direction r.  A view -- no synchronisation; later steps overwrite it."""
        a = self._arena
        if a is None or a["lamb"] is None or not a["lamb_stepped"]:
            raise RuntimeError("trust_ratios(): no step has been taken with trust_ratio = True")
        return a["lamb"][2]

    def _lamb_update(self, c):
        """The three LAMB launches of launch class `c` on the current stream."""
        a = self._arena
        partials, trust, report = self.lamb_buffers()
        clip = self._clip_record()
        part = partials[2 * c["rec0"]:2 * (c["rec0"] + c["n"])]
        ops.lamb_stage1(a["p"], self._grad_operand(), a["m"], a["v"], c["table"], c["n"], c["hyper"], part, self.grad_scale, clip)
        ops.lamb_trust(part, c["table"], c["n"], c["tensor_first"], c["rec_tensor"], c["ntensors"], trust, report, clip)
        ops.lamb_stage2(a["p"], a["m"], a["v"], c["table"], c["n"], c["hyper"], trust, c["rec_tensor"], clip, p_bf16=a["pb"])
        a["lamb_stepped"] = True

    # ---- per-tensor gradient / weight statistics ----------------------------------------------------------------------
    def stats_setting(self) -> bool:
        """tensor_stats, validated: anything but a bool raises ValueError."""
        if not isinstance(self.tensor_stats, bool):
            raise ValueError(f"tensor_stats must be True or False, got {self.tensor_stats!r}")
        return self.tensor_stats

    def stats_buffers(self):
        """(partials, bad, stats, counts): four fp32 partials and two int32 counts per CHUNK record of the arena, one report row
        [grad norm, max |g|, weight norm, max |p|] (fp32) and one row [non-finite g, non-finite p, steps with a non-finite g] (int64) per
        arena tensor (_feature_buffers: None before the arena exists; the sticky third count restarts with the arena, as skipped_steps()
        does)."""
        def alloc(a, dev):
            n, nt = self._arena_records(), len(a["index"])
            a["stats_stepped"] = False
            return (torch.zeros(4 * n, dtype=torch.float32, device=dev), torch.zeros(2 * n, dtype=torch.int32, device=dev),
                    torch.zeros(nt, 4, dtype=torch.float32, device=dev), torch.zeros(nt, 3, dtype=torch.int64, device=dev))
        return self._feature_buffers("stats", "tensor_stats", "stats_buffers", alloc)

    def tensor_stats_launch(self):
        """The two statistics launches of every launch class over its whole chunk table, on the current stream.  Belongs behind the step's
        update (and EMA) launches: g is then the gradient the update read -- the updates never write it --, p the parameter it wrote."""
        a = self._arena
        partials, bad, stats, counts = self.stats_buffers()
        g = self._grad_operand()
        for c in self._launch:
            part, cnt = partials[4 * c["rec0"]:4 * (c["rec0"] + c["n"])], bad[2 * c["rec0"]:2 * (c["rec0"] + c["n"])]
            ops.tensor_stats_stage1(a["p"], g, c["table"], c["n"], part, cnt)
            ops.tensor_stats_stage2(part, cnt, c["n"], c["tensor_first"], c["rec_tensor"], c["ntensors"], self.grad_scale, stats, counts)
        a["stats_stepped"] = True

    def tensor_stats_report(self):
        """(stats [tensors in arena order (arena_layout(), tensor_names()), 4] fp32, counts [same rows, 3] int64) of the last step with
        tensor_stats on: stats rows are [||g||, max |g|, ||p||, max |p|] over the finite elements, g being the gradient the update read
        (after the exchange, unclipped, times grad_scale: what grad_norm() describes) and p the parameter after the step; counts rows are
        [non-finite elements of g, of p, steps so far with a non-finite g].  Device views -- no synchronisation; later steps overwrite them."""
        a = self._arena
        if a is None or a["stats"] is None or not a["stats_stepped"]:
            raise RuntimeError("tensor_stats_report(): no step has been taken with tensor_stats = True")
        return a["stats"][2], a["stats"][3]

    def tensor_names(self, model) -> List:
        """The names of `model.named_parameters()` in arena order: the rows of tensor_stats_report() and trust_ratios().  A tied parameter
        carries its first name; a member that `model` does not hold gets None."""
        if self._arena is None:
            raise RuntimeError("tensor_names(): no step has been taken yet: the arena does not exist")
        names = {id(p): n for n, p in model.named_parameters()}
        return [names.get(pid) for pid in self._arena["index"]]

    def nonfinite_tensors(self, model) -> Dict[str, tuple]:
        """{parameter name: (non-finite gradient elements in the last step, steps so far with a non-finite gradient)} for every arena
        tensor whose gradient has been non-finite at least once since the arenas were built.  Reads the device counts: SYNCHRONISES."""
        counts = self.tensor_stats_report()[1].cpu()
        return {name: (int(row[0]), int(row[2])) for name, row in zip(self.tensor_names(model), counts) if int(row[2]) > 0}

    # ---- EMA of the weights --------------------------------------------------------------------------------------------
    def ema_setting(self):
        """None with the feature off, else (ema_decay as a float, ema_warmup).  Raises ValueError for an ema_decay that is not a real number
        strictly inside (0, 1) and for an ema_warmup that is not a bool."""
        if not isinstance(self.ema_warmup, bool):
            raise ValueError(f"ema_warmup must be True or False, got {self.ema_warmup!r}")
        d = self.ema_decay
        if d is None:
            return None
        if isinstance(d, bool) or not isinstance(d, numbers.Real):
            raise ValueError(f"ema_decay must be None or a number strictly inside (0, 1), got {d!r}")
        d = float(d)
        if not 0.0 < d < 1.0:          # (also a NaN)
            raise ValueError(f"ema_decay must be strictly inside (0, 1), got {d!r}")
        return d, self.ema_warmup

    def ema_weight(self, n=None) -> float:
        """The weight w of the next EMA update, e += w (p - e): float32(1 - decay_eff), decay_eff = min(decay, (1 + n) / (10 + n)) with
        warm-up and `decay` without, computed in double and rounded once to fp32 (returned as a Python float holding that fp32 value);
        n = `ema_updates` unless given.  0.0 with the feature off."""
        setting = self.ema_setting()
        if setting is None:
            return 0.0
        decay, warm = setting
        n = self.ema_updates if n is None else int(n)
        if warm:
            decay = min(decay, (1.0 + n) / (10.0 + n))
        return struct.unpack("<f", struct.pack("<f", 1.0 - decay))[0]

    def _stash_ema(self, arena):
        """Before `arena` is dropped: keep views of its shadow per parameter for the arena that replaces it."""
        if arena is not None and arena.get("ema") is not None:
            for pid, (o, n) in arena["index"].items():
                self._ema_carry[pid] = arena["ema"][o:o + n]

    def ema_buffers(self):
        """The shadow arena: fp32, the size and offsets of the parameter arena.  Created on first use -- only with the feature on -- as a copy
        of the parameter arena at that moment; shadow values carried over from a previous arena or handed to load_ema() replace the copy for
        their parameters.  Not part of state_dict.  None before the arena exists."""
        def alloc(a, dev):
            with torch.no_grad():
                return a["p"].clone()
        a = self._arena
        if self._feature_buffers("ema", "ema_decay", "ema_buffers", alloc) is None:
            return None
        if self._ema_carry:
            with torch.no_grad():
                for pid in [pid for pid in self._ema_carry if pid in a["index"]]:
                    o, n = a["index"][pid]
                    t = self._ema_carry.pop(pid)
                    if t.numel() != n:
                        raise RuntimeError(f"EMA shadow of {t.numel()} elements for a parameter of {n}")
                    a["ema"][o:o + n].copy_(t.reshape(-1))
            self._ema_carry.clear()          # what is left belongs to no member: should it join later, it starts from its current value
        return a["ema"]

    def _ema_if_any(self):
        """The shadow arena when it exists or the feature is on (then created), else None: reading never allocates with the feature off."""
        a = self._arena
        if a is None or (a["ema"] is None and self.ema_setting() is None):
            return None
        return self.ema_buffers()

    def _ema_members(self):
        a = self._arena
        return [] if a is None else [p for g in self.param_groups for p in g["params"] if id(p) in a["index"]]

    def ema_parameters(self):
        """{parameter: its view into the shadow arena} for every arena member (parameters that never received a gradient are absent:
        their EMA is the parameter itself).  Empty before the arena exists.  While swapped (swap_ema) the views hold the training weights."""
        e = self._ema_if_any()
        out = {}
        if e is not None:
            for p in self._ema_members():
                o, n = self._arena["index"][id(p)]
                out[p] = e[o:o + n].view(p.shape)
        return out

    def ema_state_dict(self, model):
        """OrderedDict with exactly the keys of `model.state_dict()`: cloned shadow values for arena members, cloned current values for
        everything else (parameters without a gradient, buffers) -- the file to evaluate or ship."""
        if self._ema_swapped:
            raise RuntimeError("ema_state_dict(): the weights are swapped with the shadow (swap_ema / ema_weights): swap back first")
        e = self._ema_if_any()
        index = {} if self._arena is None else self._arena["index"]
        out = OrderedDict()
        for k, v in model.state_dict(keep_vars=True).items():
            rng = index.get(id(v))
            out[k] = v.detach().clone() if (e is None or rng is None) else e[rng[0]:rng[0] + rng[1]].view(v.shape).clone()
        return out

    def ema_checkpoint(self, model):
        """The value of the checkpoint key `ytvln_ema_state` (None with the feature off): {"decay", "warmup", "updates", "shadow": {name
        in model.state_dict(): cloned shadow tensor of that arena member}}."""
        setting = self.ema_setting()
        if setting is None:
            return None
        if self._ema_swapped:
            raise RuntimeError("ema_checkpoint(): the weights are swapped with the shadow (swap_ema / ema_weights): swap back first")
        e = self.ema_buffers()
        shadow = OrderedDict()
        if e is not None:
            for k, v in model.state_dict(keep_vars=True).items():
                rng = self._arena["index"].get(id(v))
                if rng is not None:
                    shadow[k] = e[rng[0]:rng[0] + rng[1]].view(v.shape).clone()
        for k, v in model.state_dict(keep_vars=True).items():          # loaded, not yet adopted (no step since): carried through
            if k not in shadow and id(v) in self._ema_carry:
                shadow[k] = self._ema_carry[id(v)].detach().clone().view(v.shape)
        return {"decay": setting[0], "warmup": setting[1], "updates": int(self.ema_updates), "shadow": shadow}

    def load_ema(self, state, model):
        """Take the shadow and the update count of a checkpoint's `ytvln_ema_state` (names are those of `model.state_dict()`).  The tensors
        stay pending until the shadow arena exists: ema_buffers() adopts them (the first step with the feature on; at once when the shadow
        is already there).  `ema_decay` / `ema_warmup` are settings like max_grad_norm: they come from the attributes, not from the file."""
        if self._ema_swapped:
            raise RuntimeError("load_ema(): the weights are swapped with the shadow (swap_ema / ema_weights): swap back first")
        named = model.state_dict(keep_vars=True)
        for k, t in state["shadow"].items():
            if k not in named:
                raise KeyError(f"load_ema: the model has no tensor named {k!r}")
            if tuple(t.shape) != tuple(named[k].shape):
                raise RuntimeError(f"load_ema: {k}: shadow of shape {tuple(t.shape)} for a tensor of shape {tuple(named[k].shape)}")
            self._ema_carry[id(named[k])] = t.detach().to(dtype=torch.float32)
        self.ema_updates = int(state["updates"])
        if self._arena is not None and self._arena["ema"] is not None:
            self.ema_buffers()

    def swap_ema(self):
        """Exchange the parameter arena and the shadow in place, ytvln_ema_swap over every launch class on the current stream; the bf16
        weight copy (bf16_arena()) is refreshed by the same pass.  Only contents move: parameter views, arena slots and captured graphs
        stay valid.  Until the next swap_ema() the optimizer refuses to step."""
        a = self._arena
        if a is None or self._launch is None or a["ema"] is None:
            raise RuntimeError("swap_ema(): no step has been taken with ema_decay set")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("swap_ema() is an eager operation: not inside a capture")
        self.ema_buffers()
        for c in self._launch:
            ops.ema_swap(a["p"], a["ema"], c["table"], c["n"], p_bf16=a["pb"])
        self._ema_swapped = not self._ema_swapped

    @contextlib.contextmanager
    def ema_weights(self):
        """`with optimizer.ema_weights():` -- the model computes with the shadow weights inside the block (swap_ema() in and back out)."""
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()

    def _not_swapped(self, what):
        if self._ema_swapped:
            raise RuntimeError(f"{what}: the weights are swapped with their EMA shadow (swap_ema / ema_weights); swap back before training on")

    def _update(self, table, n, hyper, cls=None):
        a = self._arena
        # the shadow starts as the weights BEFORE the first update it follows: created (first use) ahead of the update launches
        shadow = self.ema_buffers() if self.ema_setting() is not None else None
        self._update_launches(table, n, hyper, cls)
        if shadow is not None:          # a launch of its own behind the update: element-wise, so any cut of the table will do
            ops.ema_update(a["p"], shadow, table, n, hyper, self._clip_record())

    def _update_launches(self, table, n, hyper, cls=None):
        a = self._arena
        if self.lamb_setting():
            if cls is None or table is not cls["table"]:
                raise RuntimeError("trust_ratio: the norms run over whole tensors, so the update runs over whole launch classes "
                                   "(launch_classes()), not over pieces of their chunk tables")
            return self._lamb_update(cls)
        g, clip = self._grad_operand(), self._clip_record()
        if clip is not None:
            ops.adamw_step_clip(a["p"], g, a["m"], a["v"], table, n, hyper, clip, self.grad_scale, p_bf16=a["pb"])
        elif g.dtype == torch.bfloat16:
            ops.adamw_step_gbf16(a["p"], g, a["m"], a["v"], table, n, hyper, self.grad_scale, p_bf16=a["pb"])
        else:
            ops.adamw_step(a["p"], g, a["m"], a["v"], table, n, hyper, self.grad_scale, p_bf16=a["pb"])

    def _adopt_grad(self, p):
        """A member's gradient that is not the view of its arena slot (model.zero_grad() dropped the views; the few tensors autograd
        allocates itself) is copied into the slot and becomes the view.  Callers hold torch.no_grad()."""
        fg = self._arena["g"]
        o, n = self._arena["index"][id(p)]
        if p.grad.data_ptr() != fg.data_ptr() + 4 * o:
            fg[o:o + n].copy_(p.grad.reshape(-1))
            p.grad = fg[o:o + n].view(p.shape)

    def _ensure_arena(self):
        members = self._members()
        if not members:
            return members
        if self._arena is None or self._arena["ids"] != [id(p) for _, p in members]:
            self._build_arena(members)
            return members
        base_p, index = self._arena["p"].data_ptr(), self._arena["index"]
        stale_data = False
        with torch.no_grad():
            for _, p in members:
                if p.data_ptr() != base_p + 4 * index[id(p)][0]:
                    stale_data = True
                    break
                self._adopt_grad(p)
        if stale_data:                                         # parameters were re-allocated (model.to(...)): rebuild
            self._build_arena(members)
        return members

    def _build_launch(self, members):
        classes: Dict[tuple, list] = {}
        for gi, p in members:
            classes.setdefault((gi, self.state[p]["step"]), []).append(p)
        index, dev = self._arena["index"], self._arena["p"].device
        order = {pid: k for k, pid in enumerate(index)}          # a tensor's row in the trust / report buffers: its place in the arena
        launch = []
        rec0 = 0
        for (gi, step), plist in classes.items():
            wd = float(self.param_groups[gi]["weight_decay"])
            rec, n = chunk_table([index[id(p)] + (wd,) for p in plist])
            table = torch.frombuffer(rec, dtype=torch.uint8).to(dev)
            first, rec_tensor = lamb_tables([(order[id(p)], index[id(p)][1]) for p in plist])
            assert len(rec_tensor) == n
            # hyper-parameters travel through a small ring of pinned host buffers (async H2D, no per-step stream sync);
            # an event per slot guards reuse should the host ever run a full ring ahead of the device.
            launch.append(dict(group=gi, step=step, params=plist, table=table, n=n, rec0=rec0, ntensors=len(plist),
                               tensor_first=torch.tensor(first, dtype=torch.int32).to(dev),
                               rec_tensor=torch.tensor(rec_tensor, dtype=torch.int32).to(dev),
                               hyper=torch.zeros(8, dtype=torch.float32, device=dev),
                               ring=[torch.zeros(8, dtype=torch.float32).pin_memory() for _ in range(4)],
                               events=[None] * 4, slot=0))
            rec0 += n
        self._launch = launch

    def load_state_dict(self, state_dict):
        """torch's loader replaces `state[p]["exp_avg"/"exp_avg_sq"]` with fresh tensors: drop the arenas so the next step rebuilds
        them and re-adopts the LOADED moments (otherwise the kernel would keep updating the old arena while state_dict()
        serialised the stale loaded tensors)."""
        self._not_swapped("load_state_dict()")
        super().load_state_dict(state_dict)
        # parameters / gradients keep viewing the old arenas (still valid memory) until the rebuild copies them over
        if self._arena is not None:
            self._written.clear()
        self._stash_ema(self._arena)          # the EMA shadow is not optimizer state of the file: it moves into the next arena
        self._arena = None
        self._launch = None

    # ---- the step -------------------------------------------------------------------------------------------------
    def _upload_hyper(self):
        """Host -> device upload of (beta1, beta2, eps, step_size, lr, bias correction, EMA weight) for every launch class and advance of
        the step counters.  Eager by design: under hipGraph replay (`capturing=True` steps) this is the only per-step host work."""
        ema_w = self.ema_weight()           # 0 with the EMA off
        for c in self._launch:
            g = self.param_groups[c["group"]]
            b1, b2 = g["betas"]
            t = c["step"] + 1
            step_size, bias = g["lr"], 1.0
            if g["correct_bias"]:
                step_size = step_size * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
                bias = math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
            k = c["slot"] = (c["slot"] + 1) % 4
            if c["events"][k] is not None:
                c["events"][k].synchronize()
            host = c["ring"][k]
            host[0], host[1], host[2], host[3], host[4] = b1, b2, g["eps"], step_size, g["lr"]
            host[5] = bias              # read by the LAMB launches only (trust_ratio)
            host[6] = ema_w             # read by ytvln_ema_update only (ema_decay)
            c["hyper"].copy_(host, non_blocking=True)
            c["events"][k] = torch.cuda.Event()
            c["events"][k].record()
            c["step"] = t
            for p in c["params"]:
                self.state[p]["step"] = t
        if self.ema_decay is not None:
            self.ema_updates += 1

    def _launch_kernels(self):
        now = self.capture_settings()
        if now.clip is not None:                  # norm of what the update reads -> coefficient -> clip-aware update, all in stream order
            self.clip_coef(self.sumsq_tables([(ci, c["table"], c["n"]) for ci, c in enumerate(self._launch)], 0))
        if torch.cuda.is_current_stream_capturing():
            self._captured = now
        self.launch_classes()
        if now.stats:                             # behind every update and EMA launch of the step
            self.tensor_stats_launch()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.capture_settings()           # an invalid opt-in attribute: ValueError before anything is exchanged, launched or recorded
        self._not_swapped("step()")
        if torch.cuda.is_current_stream_capturing():
            # inside a hipGraph capture of a whole training step: only the device work is recorded; the caller uploads the
            # hyper-parameters eagerly before every replay (`prepare_replay()`).  The arena must already exist.
            self._capture_ready("step()")
            self._ensure_arena()          # records the device copies that adopt the few non-arena gradients (embeddings)
            self._written.clear()
            self._launch_kernels()
            return loss
        members = self._ensure_arena()
        if not members:
            return loss
        if self._launch is None or any(self.state[c["params"][0]]["step"] != c["step"] for c in self._launch):
            self._build_launch(members)
        a = self._arena
        self._written.clear()                                   # gradients are consumed: slots may be written directly again
        if getattr(self, "grad_sync", None) is not None:      # data-parallel gradient exchange (ytvln/distributed.py)
            self.grad_sync(a["g"], [(p,) + a["index"][id(p)] for _, p in members])
        self._upload_hyper()
        self._launch_kernels()
        return loss

    # -- two-phase capture for data-parallel runs (ytvln.distributed.GraphedTrainStep): the gradient exchange sits between the
    #    "gradients are complete in the arena" point and the update, and stays outside any graph.
    def _capture_ready(self, what, same_members=True):
        """The preconditions of recording a step: a capture runs, an eager step built the arena, and (`same_members`) its members are unchanged."""
        if not torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{what} is only meaningful while capturing a hipGraph")
        if self._arena is None or self._launch is None:
            raise RuntimeError("run at least one eager optimizer step before capturing a step into a graph")
        if same_members and self._arena["ids"] != [id(p) for _, p in self._members()]:
            raise RuntimeError("the set of parameters receiving gradients changed; cannot capture")

    def capture_adopt(self):
        """Inside a capture, after backward: record the copies that bring the few non-arena gradients into the flat arena."""
        self._capture_ready("capture_adopt()")
        self._ensure_arena()

    def capture_adopt_some(self, params):
        """Inside a capture, in the middle of a phased backward: bring the gradients of `params` (complete at this point, the others may
        not exist yet) into their arena slots -- the partial form of capture_adopt()."""
        self._capture_ready("capture_adopt_some()", same_members=False)
        with torch.no_grad():
            for p in params:
                if p.grad is not None and id(p) in self._arena["index"]:
                    self._adopt_grad(p)

    # -- the update in pieces (ytvln.distributed.GraphedTrainStep, phased): each group of arena ranges is updated as soon as ITS gradients are
    #    complete and exchanged, on the communication stream, under the rest of the backward pass.  The kernel is element-wise over a chunk
    #    table, so cutting the table changes no bit.
    def group_tables(self, group_slices, owner=None):
        """[per group: [(launch class index, chunk table on the device, number of chunks)]] for groups given as lists of (lo, hi) ranges of
        the flat arena (whole parameter slots).  Cached on `owner` until the launch classes are rebuilt."""
        if self._arena is None or self._launch is None:
            raise RuntimeError("run at least one eager optimizer step first")
        cache = getattr(owner, "_group_tables_cache", None) if owner is not None else None
        if cache is not None and cache[0] is self._launch:
            return cache[1]
        index, dev = self._arena["index"], self._arena["p"].device
        starts = sorted((lo, hi, k) for k, sl in enumerate(group_slices) for lo, hi in sl)

        def group_of(o):
            for lo, hi, k in starts:
                if lo <= o < hi:
                    return k
            return None
        out = [[] for _ in group_slices]
        for ci, c in enumerate(self._launch):
            wd = float(self.param_groups[c["group"]]["weight_decay"])
            runs = [[] for _ in group_slices]
            for p in c["params"]:
                o, numel = index[id(p)]
                k = group_of(o)
                if k is None:
                    raise RuntimeError("a parameter of the arena belongs to no gradient group: cannot split the update")
                runs[k].append((o, numel, wd))
            for k, r in enumerate(runs):
                rec, n = chunk_table(r)
                if n:
                    out[k].append((ci, torch.frombuffer(rec, dtype=torch.uint8).to(dev), n))
        if owner is not None:
            owner._group_tables_cache = (self._launch, out)
        return out

    def launch_classes(self):
        """The update of every launch class over its whole chunk table, on the current stream: the form the LAMB update (trust_ratio) needs."""
        self._not_swapped("launch_classes()")
        for c in self._launch:
            self._update(c["table"], c["n"], c["hyper"], c)

    def launch_tables(self, tables):
        """The fused AdamW kernels of one group, on the current stream (hyper-parameters come from prepare_replay())."""
        self._not_swapped("launch_tables()")
        for ci, table, n in tables:
            self._update(table, n, self._launch[ci]["hyper"])

    def group_update(self, tables_k):
        """The gradients of one group (`tables_k`: its entry of group_tables()) are complete and exchanged: launch, on the current stream,
        what can be done now.  Plain AdamW (with or without the EMA): the group's update.  With clipping on: only its sums of squares, into
        the next free partial slots -- the coefficient needs every group's.  With the trust ratio on: nothing -- its launches run over
        whole launch classes, which the groups cut across.  finish_group_step() does the rest."""
        if self.clip_settings() is not None:
            self._group_slot = self.sumsq_tables(tables_k, self._group_slot)
        elif not self.lamb_setting():
            self.launch_tables(tables_k)

    def finish_group_step(self, tables):
        """After group_update() of the last group of `tables` (group_tables()), on the current stream: the clip coefficient over the slots
        the groups filled and every update they deferred (in group order, or per launch class with the trust ratio on), then the per-tensor
        statistics behind the step's last update.  Gradients are consumed: arena slots may be written directly again."""
        now = self.capture_settings()
        if now.clip is not None:
            self.clip_coef(self._group_slot)
        if now.lamb:
            self.launch_classes()
        elif now.clip is not None:
            for tables_k in tables:
                self.launch_tables(tables_k)
        if now.stats:
            self.tensor_stats_launch()
        self._written.clear()

    def arena_range(self, p):
        """(offset, numel) of a parameter's slot in the flat arenas, or None."""
        return None if self._arena is None else self._arena["index"].get(id(p))

    def capture_update(self):
        """Inside a capture: record the fused AdamW kernels (hyper-parameters come from prepare_replay())."""
        self._not_swapped("capture_update()")
        if not torch.cuda.is_current_stream_capturing():
            raise RuntimeError("capture_update() is only meaningful while capturing a hipGraph")
        self._written.clear()
        self._launch_kernels()

    def flat_grad(self):
        """The flat fp32 gradient arena (None before the first optimizer step)."""
        return None if self._arena is None else self._arena["g"]

    def prepare_replay(self):
        """Call before each replay of a captured training step (after scheduler.step() set the new learning rate).  The captured step
        carries the clipping settings, trust_ratio, EMA on / off and tensor_stats it was recorded with: raises if one of them changed since
        (the EMA's decay and warm-up travel by value and may change freely)."""
        self._not_swapped("prepare_replay()")
        if self._captured is not None:
            now = self.capture_settings()
            changed = [f"{_SETTING_ATTRS[f]} (captured {was!r}, now {is_!r})"
                       for f, was, is_ in zip(now._fields, self._captured, now) if was != is_]
            if changed:
                raise RuntimeError(f"changed since the step was captured: {'; '.join(changed)}: the graph holds the old launches -- "
                                   "capture the step again")
        self._group_slot = 0
        self._upload_hyper()

    def zero_grad(self, set_to_none: bool = True):
        """Drop the gradients (`p.grad = None`).  With the arena in place the next backward writes weight gradients straight
        into their arena slots (ytvln.ops._direct_grad) and autograd adopts those views, so no memset and no accumulation
        pass is needed; the few small tensors that arrive as separate allocations (biases, LayerNorm, embeddings) are
        copied into their slots at the next step().  `set_to_none=False` zeroes the arena in place and keeps the views."""
        if self._arena is not None:
            self._written.clear()
        if self._arena is None or set_to_none:
            return super().zero_grad(set_to_none=True)
        self._arena["g"].zero_()
