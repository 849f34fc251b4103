"""torch.autograd.Function wrappers over the C ABI (include/ytvln.h).

PyTorch supplies device memory, the current HIP stream and the autograd graph; every FLOP / byte of the hot path runs in
libytvln.so.  All wrappers require CUDA(HIP) fp32 tensors -- there is no CPU or eager-PyTorch fallback.
"""
from __future__ import annotations

import contextlib
import math
import ctypes
import os
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import ACT_SWISH, EPI_GELU, EPI_MUL_DGELU, EPI_NONE, EPI_RELU, GEMM_A_ZERO_PADDED, GEMM_SPLIT_BF16X3, call

Tensor = torch.Tensor
# "swish" is not a GEMM epilogue: the projection runs with EPI_NONE and ytvln_act_fwd_* follows (LinearFn, either format)
_ACT = {"none": EPI_NONE, None: EPI_NONE, "gelu": EPI_GELU, "relu": EPI_RELU, "swish": ACT_SWISH}


# ------------------------------------------------------------------------------------------------------------------
# plumbing helpers
# ------------------------------------------------------------------------------------------------------------------
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> int:
    """Raw hipStream_t of torch's current stream (the C accessor avoids building Stream objects ~2500 times per step)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[Tensor], offset_elems: int = 0):
    if t is None:
        return None
    return t.data_ptr() + 4 * offset_elems


def _check(t: Tensor, name: str, dtype=torch.float32):
    if not t.is_cuda:
        raise RuntimeError(f"ytvln.ops: `{name}` must live on the GPU (no CPU fallback); got device {t.device}")
    if t.dtype != dtype:
        raise RuntimeError(f"ytvln.ops: `{name}` must be {dtype}; got {t.dtype}")


def _i64(t: Tensor, name: str) -> Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"ytvln.ops: `{name}` must live on the GPU")
    if t.dtype != torch.int64:
        t = t.to(torch.int64)
    return t.contiguous()


# ------------------------------------------------------------------------------------------------------------------
# dropout RNG state: (seed, forward counter) in device memory + host-side site ids
# ------------------------------------------------------------------------------------------------------------------
class DropoutState:
    """Philox key material for one forward pass.  `tensor` is an int64[2] DEVICE tensor (seed, counter) that the kernels
    read; every dropout site of the pass takes the next `site` id.  Backward regenerates masks from (tensor, site).

    Seeding follows the reference's `set_seed` (utils/misc.py:37-45: `torch.manual_seed(seed + local_rank)`): unless
    `manual_seed()` was called explicitly, the per-device stream is keyed by `torch.initial_seed()` at the moment the first
    training-mode forward creates it, so different `--seed`s / ranks draw independent masks.  `get_state()` / `set_state()`
    carry (seed, counter) through checkpoints so a resumed run continues the stream instead of replaying it."""

    _global = {}
    seed = None          # None: derive from torch.initial_seed() when a device's stream is first created

    def __init__(self, device):
        device = torch.device(device)
        g = DropoutState._global.get(device)
        if g is None:
            seed = DropoutState.seed if DropoutState.seed is not None else (torch.initial_seed() & 0x7FFFFFFFFFFFFFFF)
            g = torch.tensor([seed, 0], dtype=torch.int64, device=device)
            DropoutState._global[device] = g
        self.tensor = g.clone()          # frozen copy for this forward (and its backward)
        g[1] += 1                        # device-side increment: graph-capturable, no host sync
        self._site = 0

    def next_site(self) -> int:
        self._site += 1
        return self._site

    @classmethod
    def manual_seed(cls, seed):
        """Explicit seed for every device's stream (restarts the counters).  `None` returns to following torch.initial_seed()."""
        cls.seed = None if seed is None else int(seed) & 0x7FFFFFFFFFFFFFFF
        cls._global.clear()

    @classmethod
    def get_state(cls) -> dict:
        """{device string: (seed, counter)} of every mask stream THIS process owns (one per device it ran a training-mode forward on; one
        process per GPU: normally a single entry) -- one device->host read per entry, at checkpoint time only."""
        return {str(dev): tuple(int(v) for v in t.tolist()) for dev, t in cls._global.items()}

    @classmethod
    def set_state(cls, state: dict, device=None) -> None:
        """Restore a saved stream onto `device` -- default: the device of the one stream this process already owns, else the caller's
        current device -- whatever device string the checkpoint carries (one process per GPU: a checkpoint written by rank 0 on cuda:0 is
        resumed by rank k on cuda:k and must not make it touch cuda:0 -- ADVICE r2).  The entry saved under the target's own device string
        is preferred; otherwise the first saved entry is taken and, when the device indices differ, its seed is shifted by the index
        difference so that the ranks' mask streams stay distinct the way `set_seed(seed + local_rank)` made them (utils/misc.py:37-45).
        Pass the model's device when it is not the current one."""
        if not state or not torch.cuda.is_available():
            return
        if device is not None:
            cur = torch.device(device)
            if cur.type == "cuda" and cur.index is None:
                cur = torch.device("cuda", torch.cuda.current_device())
        elif len(cls._global) == 1:
            cur = next(iter(cls._global))
        else:
            cur = torch.device("cuda", torch.cuda.current_device())
            if cls._global and cur not in cls._global:
                import warnings
                warnings.warn(f"DropoutState.set_state: restoring onto the current device {cur} while this process owns streams on "
                              f"{sorted(map(str, cls._global))}; pass device= to choose")
        key = str(cur) if str(cur) in state else sorted(state)[0]
        seed, counter = state[key]
        saved = torch.device(key)
        shift = (cur.index or 0) - (saved.index or 0) if saved.type == "cuda" else 0
        cls._global[cur] = torch.tensor([(int(seed) + shift) & 0x7FFFFFFFFFFFFFFF, int(counter)], dtype=torch.int64, device=cur)


# ------------------------------------------------------------------------------------------------------------------
# two HIP streams for the two streams of the model
# ------------------------------------------------------------------------------------------------------------------
class TwoStream:
    """The text stream and the image stream of ViLBERT are independent between co-attention layers (vilbert.py:737-811: T0..T5 need
    nothing from the image side, V_i and T_6+i both start from the outputs of co-layer i, and behind the co-attention itself each side's
    BertBiOutput + FFN is its own chain).  With `set_two_stream(True)` the text-side launches go to a second HIP stream: the 4480-row
    text GEMMs fill 82 % of the chip's CUs in their last round of tiles and the small LayerNorm / attention launches of that side leave
    most of it idle -- the other side's workgroups take those CUs.  Every kernel is still the same deterministic launch and the Python
    call order (hence every dropout site id) is unchanged, so results are bit-identical to the one-stream run; autograd runs each
    node's backward on the stream of its forward, so the backward pass splits the same way, and under hipGraph capture the two
    streams become two branches of the graph.

    Allocator safety: a tensor produced on one stream and read on the other is `record_stream`ed by `side()` / `join()` (gradients
    crossing streams in the backward pass are recorded by the autograd engine)."""

    enabled = True
    _side = {}
    _last_main = {}      # device -> the stream the last region was opened on
    _quiet = False
    active = False
    main = None          # the stream the region was opened on
    fp = None            # event on the main stream that covers everything the text side may read from it

    @classmethod
    def side_stream(cls, device) -> "torch.cuda.Stream":
        device = torch.device(device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        s = cls._side.get(device)
        if s is None:
            s = cls._side[device] = torch.cuda.Stream(device=device)
        return s

    @classmethod
    def begin(cls, device) -> bool:
        """Start a forked region on the caller's current stream; False when the mode is off or a region is already open."""
        if not cls.enabled or cls.active or torch.device(device).type != "cuda":
            return False
        if not cls._quiet:
            # a parameter both sides use (the word embedding tied to the language decoder) gets gradients from both streams by design: the
            # engine orders them; its advice to "initialise DDP under the same stream" does not apply
            quiet = getattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch", None)
            if quiet is not None:
                quiet(False)
            cls._quiet = True
        cls.active = True
        cls.main = torch.cuda.current_stream()
        cls._last_main[cls.main.device] = cls.main
        cls.mark()
        return True

    @classmethod
    def mark(cls) -> None:
        """New fork point: the text side may read whatever the main stream has been given up to here."""
        if cls.active:
            ev = torch.cuda.Event()
            ev.record(cls.main)
            cls.fp = ev

    @classmethod
    def side(cls, *inputs):
        """Context: launches inside go to the side stream, ordered behind the last fork point.  `inputs` = tensors the body reads that
        were produced on the main stream."""
        if not cls.active:
            return contextlib.nullcontext()
        s = cls.side_stream(cls.main.device)
        s.wait_event(cls.fp)
        for t in inputs:
            if t is not None and t.is_cuda:
                t.record_stream(s)
        return torch.cuda.stream(s)

    @classmethod
    def join(cls, *outs) -> None:
        """The main stream waits for the text side; `outs` = tensors produced there that the main stream reads next."""
        if not cls.active:
            return
        main = cls.main
        main.wait_stream(cls.side_stream(main.device))
        for t in outs:
            if t is not None and t.is_cuda:
                t.record_stream(main)

    @classmethod
    @contextlib.contextmanager
    def shared_write(cls):
        """Context for a write to memory that BOTH sides read and that is not part of the forward's dataflow (the lazily created / refreshed
        bf16 copy of the weight arena): inside a two-stream region the write is enqueued on the main stream, becomes the new fork point,
        and a caller that is currently on the side stream waits for it too.  Outside a region: a plain pass-through."""
        if not cls.active:
            yield
            return
        cur = torch.cuda.current_stream()
        with torch.cuda.stream(cls.main):
            yield
        cls.mark()
        if cur != cls.main:
            cur.wait_event(cls.fp)

    @classmethod
    def gather_streams(cls) -> None:
        """Make the CURRENT stream wait for both sides of the model.  For code that runs inside a backward pass (a gradient hook runs on the
        stream of the parameter it fires for) and is about to hand a block of gradients that came from BOTH sides to something ordered
        behind the current stream only: the bucket collectives of ytvln.distributed."""
        if not cls.enabled or not cls._side or torch.cuda.is_current_stream_capturing():
            return
        cur = torch.cuda.current_stream()
        for s in (cls._side.get(cur.device), cls._last_main.get(cur.device)):
            if s is not None and s != cur:
                cur.wait_stream(s)

    @classmethod
    def join_backward(cls) -> None:
        """Call after a backward pass that ran (partly) on the side stream and before anything reads the gradients on the current
        stream.  The autograd engine joins the streams of the leaves it ran at the end of a backward pass, but a parameter's
        AccumulateGrad node keeps the stream it was CREATED on: one pinned earlier on the null stream (a post-accumulate hook registered
        before the model ran) takes no part in a stream capture, and the text side's last kernels would then have no edge to the
        capturing stream.  This join does not depend on where those nodes live.  No-op when the side stream has nothing in flight for
        the current capture."""
        if not cls.enabled or not cls._side or not torch.cuda.is_available():
            return
        cur = torch.cuda.current_stream()
        s = cls._side.get(cur.device)
        if s is None:
            return
        if torch.cuda.is_current_stream_capturing():
            with torch.cuda.stream(s):
                if not torch.cuda.is_current_stream_capturing():
                    return
        cur.wait_stream(s)

    @classmethod
    def end(cls, *outs) -> None:
        cls.join(*outs)
        cls.active = False
        cls.fp = cls.main = None


def set_two_stream(flag: bool) -> None:
    """Text-side launches on a second HIP stream (see TwoStream).  Process-wide switch, read at the start of a model forward."""
    TwoStream.enabled = bool(flag)


def get_two_stream() -> bool:
    return TwoStream.enabled


# ------------------------------------------------------------------------------------------------------------------
# GEMM primitives
# ------------------------------------------------------------------------------------------------------------------
_WS_CACHE = {}


_MATMUL_PRECISION = "fp32"


def set_matmul_precision(mode: str) -> None:
    """"fp32" (default, the reference's arithmetic: v_mfma_f32_32x32x2_f32), "bf16" or "fp32x3".
    "bf16" (BASELINE configs[4]): the bf16-RESIDENT path -- hidden states, their gradients and a copy of the weights live in HBM as bf16;
    projections (ytvln_gemm_bf16) and attention (ytvln_attn_*_bf16) read them in place and write bf16, LayerNorm reads / writes bf16 rows;
    accumulation, softmax, LayerNorm statistics, logits, losses, master weights, weight gradients and the optimizer stay fp32.
    "fp32x3": dense projections keep fp32 operands and split every value exactly into three bf16 terms in registers; each product is
    accumulated in fp32 from the six largest cross terms on the bf16 matrix instruction (YTVLN_GEMM_SPLIT_BF16X3: error per product
    of the order of one fp32 rounding).  Attention and everything else as in "fp32".  Process-wide switch, read at call time."""
    global _MATMUL_PRECISION
    if mode not in ("fp32", "bf16", "fp32x3"):
        raise ValueError(f"matmul precision must be 'fp32', 'bf16' or 'fp32x3', got {mode!r}")
    _MATMUL_PRECISION = mode


def get_matmul_precision() -> str:
    return _MATMUL_PRECISION


def _bf16_eligible(M: int, N: int, K: int) -> bool:
    """bf16 mode: does a projection whose INPUT arrives as fp32 (network inputs, pooled vectors) enter the bf16-resident path?  Large ones
    do (the region-feature projection); the one- and two-column heads on the pooled vectors stay on the fp32 kernels."""
    return _MATMUL_PRECISION == "bf16" and M >= 64 and N >= 64 and K >= 64


def _gemm(A, lda, transA, B, ldb, transB, C, ldc, M, N, K, bias=None, aux=None, ldaux=0, epi=EPI_NONE, beta=0.0, flags=0, rowsum=None, live=None,
          rows=None):
    """fp32 operands (native fp32 matrix instruction, or the three-bf16-term form under "fp32x3").  `rowsum` = an [M] tensor that should
    receive sum_k op(A)[m, k] (the bias gradient riding on a weight-gradient GEMM, ytvln_gemm_f32_rowsum); returns True when the launch
    produced it, False when the caller has to run `colsum` itself.  `live` = the LiveRows of the K rows a weight-gradient launch (transA = 1)
    contracts over: rows of A outside the list are exact zeros (ytvln_gemm_f32_live).  `rows` = the LiveRows (with `perm`) of the M rows a
    forward / input-gradient launch (transA = 0) computes: the rows behind the count come back as zeros (beta = 0) or untouched
    (ytvln_gemm_f32_rows); a hint equal to M means "every row is expected to be listed" and launches the plain form."""
    sk = _lib.option("GEMM_SK") != 0          # the persistent kernel (opt-in): its partial-tile scratch and control block exist only then
    by_rows = (rows is not None and rows.perm is not None and not transA and rows.rows == M and rows.hint < M and rowsum is None
               and _MATMUL_PRECISION == "fp32")
    key = (M, N, K, epi, sk, "rows", rows.hint) if by_rows else (M, N, K, epi, sk)
    need = _WS_CACHE.get(key)
    if need is None:
        lib = _lib.load()
        need = _WS_CACHE[key] = int(lib.ytvln_gemm_rows_workspace_elems(M, N, K, epi, rows.hint) if by_rows
                                    else lib.ytvln_gemm_workspace_elems(M, N, K, epi))
    ws = torch.empty(need, dtype=torch.float32, device=C.device) if need else None      # split-K / stream-K scratch (caching allocator)
    if _MATMUL_PRECISION == "fp32x3":          # (never a row-listed launch: those are fp32 only)
        flags = int(flags) | GEMM_SPLIT_BF16X3
    # the arguments every entry point starts with
    head = (_ptr(A), lda, int(transA), _ptr(B), ldb, int(transB), _ptr(C), ldc, _ptr(bias), _ptr(aux), ldaux, M, N, K, epi, float(beta),
            _ptr(ws), need, int(flags))
    if by_rows:
        call("ytvln_gemm_f32_rows", *head, rows.perm.data_ptr(), rows.count.data_ptr(), rows.hint, _stream())
        return False
    ctl = _sk_ctl(C.device) if sk else None
    done = ctypes.c_int(0)
    rowsum_out = (_ptr(rowsum), ctypes.byref(done) if rowsum is not None else None)
    if live is not None and transA and not transB and live.rows == K and _MATMUL_PRECISION == "fp32":
        call("ytvln_gemm_f32_live", *head, *rowsum_out, live.idx.data_ptr(), live.count.data_ptr(), _stream())
    else:
        call("ytvln_gemm_f32_sk", *head, *rowsum_out, _ptr(ctl), _stream())
    return bool(done.value)


class LiveRows:
    """ytvln_live_rows_list's outputs for one padding mask: `idx` [rows + 32] int32 (the valid rows, ascending, then one padded row repeated),
    `count` [1] int32 -- device tensors -- and the host integer `rows`.  With `perm` [rows] int32 (ytvln_live_rows_perm: the valid rows, then
    the padded rows, both ascending) the input-gradient GEMMs of the scope compute the listed rows only -- dY is zero on the others, so nothing
    observable changes -- and, with `forward` set, the forward GEMMs too: the padded rows of every projection's output are then ZEROS, which
    reaches the padded rows of the model's own outputs (BertModel.forward_live_rows).  `hint` is the HOST's guess of the count for the launch
    plans (0 = none yet; equal to `rows` = expect no padding: plain launches)."""
    __slots__ = ("idx", "count", "rows", "perm", "hint", "forward")

    def __init__(self, idx, count, rows, perm=None, hint=0, forward=False):
        self.idx, self.count, self.rows, self.perm, self.hint, self.forward = idx, count, int(rows), perm, int(hint), bool(forward)

    def record_stream(self, stream) -> None:
        self.idx.record_stream(stream)
        self.count.record_stream(stream)
        if self.perm is not None:
            self.perm.record_stream(stream)


def live_rows(mask: Tensor, perm: bool = False) -> LiveRows:
    """List of the rows of `mask` (any shape; non-zero = valid).  One launch, no host sync; `perm` = one more for the permutation."""
    if not mask.is_cuda:
        raise RuntimeError(f"ytvln.ops: `mask` must live on the GPU (no CPU fallback); got device {mask.device}")
    rows = mask.numel()
    flags = (mask.reshape(-1) != 0).contiguous()          # one byte per row
    idx = torch.empty(rows + 32, dtype=torch.int32, device=mask.device)
    count = torch.empty(1, dtype=torch.int32, device=mask.device)
    call("ytvln_live_rows_list", flags.data_ptr(), rows, idx.data_ptr(), count.data_ptr(), _stream())
    pm = None
    if perm:
        pm = torch.empty(rows, dtype=torch.int32, device=mask.device)
        call("ytvln_live_rows_perm", flags.data_ptr(), rows, pm.data_ptr(), count.data_ptr(), _stream())          # (the same count again)
    return LiveRows(idx, count, rows, pm)


_LIVE_SCOPE = None          # the LiveRows of the side of the model whose projections are being called (BertModel sets it per side), or None
live_rows_probe = None      # tests: callable(dy [M, N], LiveRows), called by every backward that hands a list to its weight-gradient launch


@contextlib.contextmanager
def live_rows_scope(live: Optional[LiveRows]):
    """Projections called inside (LinearFn, FFNFn, ImageEmbedFn) contract their weight gradients over `live`: the caller's promise that the
    gradient of every such projection's output is exactly zero on the rows that are not listed.  Where the list carries `perm` their
    input-gradient GEMMs compute the listed rows only (same promise), and where it also has `forward` set their forward GEMMs do: the second
    promise is then that nothing reads the other rows of their outputs as data (a padded row is a key behind the -10000 mask)."""
    global _LIVE_SCOPE
    prev, _LIVE_SCOPE = _LIVE_SCOPE, live
    try:
        yield
    finally:
        _LIVE_SCOPE = prev


def _live_for(M: int, fmt) -> Optional[LiveRows]:
    """The list a forward keeps for its backward: fp32 rows, and the rows of the call are the rows of the scope.  (Callers ask only when an
    input needs a gradient; inside an autograd Function's forward the grad mode itself is always off.)"""
    live = _LIVE_SCOPE
    if live is None or fmt is not _F32 or live.rows != M or _MATMUL_PRECISION != "fp32":
        return None
    return live


def _live_kw(live: Optional[LiveRows], dy: Tensor) -> dict:
    """Keywords of a weight-gradient launch (none without a list: the bf16 GEMM keeps its signature)."""
    if live is None:
        return {}
    if live_rows_probe is not None:
        live_rows_probe(dy, live)
    return {"live": live}


def _rows_kw(live: Optional[LiveRows], forward: bool = False) -> dict:
    """Keywords of an input-gradient (or, `forward`, a forward) launch with transA = 0 inside the scope: the rows it may leave out."""
    return {} if live is None or live.perm is None or (forward and not live.forward) else {"rows": live}


_SK_CTL = {}


def _sk_ctl(device):
    """Control block of the persistent GEMM (ytvln_gemm_f32_sk: tickets, done counters, partial-tile flags; zero between launches).  A block
    must never be shared by two launches that can run at the same time, so there is one per device and ROLE: the side stream of
    `TwoStream` and everything else (eager, captured and replayed launches of a role are ordered among themselves).  Created outside
    stream capture; a first use inside a capture gets None = the launch-per-tile kernel."""
    pair = _SK_CTL.get(device)
    if pair is None:
        if torch.cuda.is_current_stream_capturing():
            return None
        n = int(_lib.load().ytvln_gemm_sk_ctl_elems())
        # (block of the main role, block of the side role, the stream that owns the main role = the one the first launch was enqueued on)
        pair = _SK_CTL[device] = (torch.zeros(n, dtype=torch.int32, device=device), torch.zeros(n, dtype=torch.int32, device=device), _stream())
        torch.cuda.synchronize(device)
    side = TwoStream._side.get(device)
    cur = _stream()
    if side is not None and cur == side.cuda_stream:
        return pair[1]
    # any other stream than the two roles (a user stream, a communication stream, a second graph): two launches sharing one block could run at
    # the same time -- those take the launch-per-tile kernel
    return pair[0] if cur == pair[2] else None


def colsum(x: Tensor, M: int, N: int, ld: int, out: Optional[Tensor] = None) -> Tensor:
    """Deterministic column sums of the [M, N] matrix at x (leading dimension ld) -> [N] (written into `out` if given,
    e.g. a gradient-arena slot)."""
    first = True
    while True:
        nstrips = (N + 255) // 256          # the kernel sweeps 256-column strips (16 bytes per lane) whenever N % 4 == 0
        nb = max(1, min((M + 31) // 32, max(1, 1024 // nstrips))) if first else 1      # two stages at most
        first = False
        rpb = (M + nb - 1) // nb
        nb = (M + rpb - 1) // rpb
        if nb == 1:
            res = out if out is not None else torch.empty(N, dtype=torch.float32, device=x.device)
            call("ytvln_colsum_f32", _ptr(x), ld, M, N, _ptr(res), N, rpb, _stream())
            return res
        part = torch.empty((nb, N), dtype=torch.float32, device=x.device)
        call("ytvln_colsum_f32", _ptr(x), ld, M, N, _ptr(part), N, rpb, _stream())
        x, M, ld = part, nb, N


def colsum_by_index(x: Tensor, M: int, N: int, ld: int, KT: int, idx_f32: Optional[Tensor] = None, idx_stride: int = 1,
                    idx_f32_offset: int = 0, idx_i64: Optional[Tensor] = None) -> Tensor:
    """out[k, n] = sum of rows r with idx[r] == k -> [KT, N] (KT <= 32)."""
    nstrips = (N + 63) // 64
    nb = max(1, min((M + 31) // 32, max(1, 1024 // nstrips)))
    rpb = (M + nb - 1) // nb
    nb = (M + rpb - 1) // rpb
    out = torch.empty((nb, KT, N), dtype=torch.float32, device=x.device)
    call("ytvln_colsum_by_index_f32", _ptr(x), ld, _ptr(idx_f32, idx_f32_offset) if idx_f32 is not None else None, idx_stride,
         _ptr(idx_i64) if idx_i64 is not None else None, M, N, KT, _ptr(out), rpb, _stream())
    if nb == 1:
        return out[0]
    return colsum(out, nb, KT * N, KT * N).view(KT, N)


# ------------------------------------------------------------------------------------------------------------------
# flat-arena hooks (registered by ytvln.optimization.AdamW once parameters / gradients live in flat arenas)
# ------------------------------------------------------------------------------------------------------------------
class ArenaSlot:
    """Where a parameter lives inside the optimizer's flat arenas.  Attached to the Parameter object as `_ytvln_slot` by
    ytvln.optimization.AdamW; `written` (shared per arena) records which gradient slots a GEMM has already written directly
    since the last optimizer step / zero_grad, so a weight used twice before one backward falls back to the additive path."""
    __slots__ = ("flat_p", "flat_g", "off", "numel", "written", "owner")

    def __init__(self, flat_p, flat_g, off, numel, written, owner=None):
        self.flat_p, self.flat_g, self.off, self.numel, self.written = flat_p, flat_g, off, numel, written
        self.owner = owner          # weakref to the optimizer that owns the arenas (its bf16 weight arena: bf16_arena())

    def valid_for(self, t) -> bool:
        return t.numel() == self.numel and t.data_ptr() == self.flat_p.data_ptr() + 4 * self.off


def _slot_of(t):
    sl = getattr(t, "_ytvln_slot", None)
    return sl if (sl is not None and sl.valid_for(t)) else None


def _targets_of(weight):
    """The parameters a weight operand stands for: itself, or the members of a packed (concatenated) view."""
    if isinstance(weight, torch.nn.Parameter):
        return (weight,)
    return getattr(weight, "_ytvln_pack_params", None)


def _direct_grad(targets, shape):
    """A fresh view of the flat gradient arena covering `targets` (adjacent there, none of them holding a gradient yet and
    none written directly since the last step), shaped `shape` -- the weight-gradient GEMM then writes its result straight
    into the arena and autograd's AccumulateGrad adopts the view without a copy or a read-modify-write pass.  None when the
    conditions do not hold (the caller then allocates a normal gradient tensor)."""
    if not targets:
        return None
    first = _slot_of(targets[0])
    if first is None:
        return None
    off = first.off
    for t in targets:
        sl = _slot_of(t)
        if sl is None or sl.flat_g is not first.flat_g or sl.off != off or t.grad is not None or sl.off in sl.written:
            return None
        off += sl.numel
    for t in targets:
        first.written.add(t._ytvln_slot.off)
    return first.flat_g[first.off:off].view(shape)


def _grad_buffer(targets, shape, device) -> Tensor:
    """Where a weight or bias gradient is written: its gradient-arena view (`_direct_grad`), or a fresh fp32 buffer."""
    g = _direct_grad(targets, shape)
    return g if g is not None else torch.empty(shape, dtype=torch.float32, device=device)


class PackRowsFn(torch.autograd.Function):
    """cat(params, dim=0) for the packed Q|K|V (or K|V) projection.  Once the optimizer has moved the parameters into its
    flat arena the members are adjacent in memory and the packed operand is a zero-copy view; the backward hands each member
    its row block of the packed gradient as a view."""

    @staticmethod
    def forward(ctx, *ts):
        ctx.set_materialize_grads(False)
        ctx.rows = [t.shape[0] for t in ts]
        first = _slot_of(ts[0])
        if first is not None:
            off, ok = first.off, True
            for t in ts:
                sl = _slot_of(t)
                if sl is None or sl.flat_p is not first.flat_p or sl.off != off:
                    ok = False
                    break
                off += sl.numel
            if ok:
                return first.flat_p[first.off:off].view((sum(ctx.rows),) + tuple(ts[0].shape[1:]))
        return torch.cat([t.detach() for t in ts], dim=0)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * len(ctx.rows)
        out, r0 = [], 0
        for r in ctx.rows:
            out.append(g.narrow(0, r0, r))
            r0 += r
        return tuple(out)


def pack_rows(*params):
    w = PackRowsFn.apply(*params)
    w._ytvln_pack_params = tuple(params)
    return w


# ------------------------------------------------------------------------------------------------------------------
# wide, oddly sized outputs (30522-way language logits, 1601-way vision logits) live in buffers whose leading dimension is
# rounded up to 32 floats: rows stay 16-byte aligned and their gradients can feed the LDS-DMA GEMM (zero-padded K tail).
# ------------------------------------------------------------------------------------------------------------------
import weakref as _weakref

_ZERO_PADDED = {}       # storage data_ptr -> leading dimension, for gradient buffers whose pad columns are known to be zero


def _pad_ld(n: int) -> int:
    return (n + 31) // 32 * 32 if (n >= 1024 and n % 32) else n


def _view_rows_as(rows: Tensor, ld: int, shape):
    """View a [M, N] row buffer with leading dimension ld as `shape` (= (*lead, N))."""
    shape = tuple(shape)
    if ld == shape[-1]:
        return rows.view(shape)
    strides, acc = [], ld
    for dim in reversed(shape[:-1]):
        strides.append(acc)
        acc *= dim
    return torch.as_strided(rows, shape, tuple(reversed(strides)) + (1,))


def _overlaps(a: Tensor, b: Tensor) -> bool:
    if a is None or b is None or a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr():
        return False
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


# ------------------------------------------------------------------------------------------------------------------
# the two storage formats of a hidden state.  LinearFn, FFNFn, AddLayerNormFn and _ln_bwd are written once against this description:
# everything that depends on whether rows are fp32 or bf16-resident (set_matmul_precision) is a member here and nowhere else.
# ------------------------------------------------------------------------------------------------------------------
class RowFormat:
    """fp32 rows -- the reference's arithmetic.  Operands are read where they lie; any leading dimension goes."""
    dtype = torch.float32
    suffix = "f32"                  # of ytvln_act_fwd_* / ytvln_act_bwd_* / ytvln_ln_fwd_* / ytvln_ln_bwd_*
    row_align = 1                   # elements: a strided row view is used in place when its leading dimension and address are multiples of this
    ln_bwd_f32_copy = False         # ytvln_ln_bwd_<suffix> takes a pointer for an fp32 copy of ds (rows that are fp32 serve as they are)
    exact_gelu_replay = True        # gelu(stored z) is the stored h bit for bit: FFNFn's `recompute_h` tier exists

    def gemm(self, *args, **kw):
        """(A, lda, transA, B, ldb, transB, C, ldc, M, N, K, **keywords).  Through the module attribute at call time: a timer may replace it."""
        return _gemm(*args, **kw)

    def empty(self, M: int, N: int, device) -> Tensor:
        return torch.empty((M, N), dtype=self.dtype, device=device)

    def cast(self, t: Tensor) -> Tensor:
        """t in this format."""
        return t

    def rows(self, x: Tensor, name: str) -> Tuple[Tensor, int, int, int]:
        """View x as [M, K] rows with unit inner stride; returns (tensor-keeping-storage, M, K, leading dimension)."""
        _check(x, name, self.dtype)
        K, a = x.shape[-1], self.row_align
        if x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= K and x.stride(0) % a == 0 and x.data_ptr() % (a * x.element_size()) == 0:
            return x, x.shape[0], K, x.stride(0)
        if not x.is_contiguous():
            x = x.contiguous()
        return x, x.numel() // max(K, 1), K, K

    def pad_ld(self, n: int) -> int:
        return _pad_ld(n)

    def alloc_rows(self, M: int, N: int, device, zero_pad: bool = False, kernel_zeroes_pad: bool = False):
        """[M, N] view with leading dimension pad_ld(N).  The pad columns are cleared here (`zero_pad`) or by the kernel the caller is about to
        launch (`kernel_zeroes_pad`) and then remembered as zero, or left as they are."""
        ld = self.pad_ld(N)
        if ld == N:
            return self.empty(M, N, device), N
        full = self.empty(M, ld, device)
        if zero_pad:
            full[:, N:].zero_()
        if zero_pad or kernel_zeroes_pad:
            key = full.untyped_storage().data_ptr()
            _ZERO_PADDED[key] = ld
            _weakref.finalize(full, _ZERO_PADDED.pop, key, None)      # `full` stays alive as the base of the returned view
        return full[:, :N], ld

    def grad_rows(self, dy: Tensor, M: int, N: int):
        """(dy as [M, N] rows, leading dimension, GEMM flags): keeps a padded-leading-dimension gradient in place."""
        d2 = dy.reshape(M, N)
        if d2.stride(1) == 1 and d2.stride(0) > N and d2.stride(0) % 4 == 0 and d2.data_ptr() % 16 == 0:
            known = _ZERO_PADDED.get(d2.untyped_storage().data_ptr()) == d2.stride(0) and d2.storage_offset() == 0
            return d2, d2.stride(0), (GEMM_A_ZERO_PADDED if known else 0)
        if not d2.is_contiguous():
            d2 = d2.contiguous()
        return d2, N, 0

    def weight(self, w: Tensor) -> Tuple[Tensor, int]:
        """(the GEMM operand that stands for the [out, in] master weight w, its leading dimension)."""
        return w, w.stride(0)

    def f32_rows(self, rows: Tensor, ld: int, N: int) -> Tuple[Tensor, int]:
        """(fp32 view or copy of [M, N] rows, its leading dimension) for `colsum`, where a bias gradient could not ride on the dW launch."""
        return rows, ld

    def accumulate_target(self, dres, M: int, K: int, *live):
        """The [M, K] row view of a residual-branch gradient the input-gradient GEMM may accumulate into (beta = 1), or None.
        `live`: tensors this backward still reads or that its caller may still hold (the output gradient): with dropout p = 0 AddLayerNormFn
        hands the SAME storage to the sublayer-output gradient and to the residual gradient, and accumulating in place would overwrite an
        operand that is being read -- the caller then falls back to a separate buffer + add."""
        if dres is None or dres.dtype != self.dtype or not dres.is_cuda or dres.numel() != M * K or not dres.is_contiguous():
            return None
        if any(_overlaps(dres, t) for t in live):
            return None
        return dres.view(M, K)


class _Bf16RowFormat(RowFormat):
    """The bf16-resident path (BASELINE configs[4]; set_matmul_precision("bf16")): hidden states and their gradients are bf16 rows of 8-element
    (16-byte) granularity, a GEMM reads the bf16 copy of a weight, and padding up to a leading dimension must be ZERO."""
    dtype = torch.bfloat16
    suffix = "bf16"
    row_align = 8
    ln_bwd_f32_copy = True
    exact_gelu_replay = False       # z is stored rounded to bf16, and bf16(gelu(float(bf16 z))) is not the stored h

    def gemm(self, *args, **kw):
        return _gemm_bf16(*args, **kw)

    def cast(self, t: Tensor) -> Tensor:
        """fp32 values entering the path (network inputs, gradients coming back from the fp32 heads) are rounded once."""
        return cast_bf16(t) if t.dtype == torch.float32 else t

    def pad_ld(self, n: int) -> int:
        return _pad8(n)

    def grad_rows(self, dy: Tensor, M: int, N: int):
        """bf16 gradients with a padded leading dimension come from the loss kernels (ytvln_ce_bwd_bf16 / ytvln_kl_bwd_bf16: zero padding written
        by the kernel) and are used in place; fp32 gradients (the small heads on the pooled vectors) are cast; anything unaligned is repacked
        into a zero-padded buffer."""
        d2 = self.cast(dy.reshape(M, N)).reshape(M, N)
        if d2.stride(1) == 1 and d2.stride(0) % 8 == 0 and d2.data_ptr() % 16 == 0 and (d2.stride(0) == N or
                                                                                       _ZERO_PADDED.get(d2.untyped_storage().data_ptr()) == d2.stride(0)):
            return d2, d2.stride(0), (GEMM_A_ZERO_PADDED if d2.stride(0) != N else 0)
        ld = _pad8(N)
        if ld == N:
            return d2.contiguous(), N, 0
        full = torch.zeros((M, ld), dtype=self.dtype, device=dy.device)
        full[:, :N].copy_(d2)
        return full[:, :N], ld, GEMM_A_ZERO_PADDED

    def weight(self, w: Tensor) -> Tuple[Tensor, int]:
        return _bf16_weight(w), w.shape[1]

    def f32_rows(self, rows: Tensor, ld: int, N: int) -> Tuple[Tensor, int]:
        return (rows.float() if ld == N else rows.contiguous().float()), N


_F32, _B16 = RowFormat(), _Bf16RowFormat()


def _format_of(t: Tensor) -> RowFormat:
    return _B16 if t.dtype == torch.bfloat16 else _F32


def _alloc_rows_bf16(M: int, N: int, device):
    """A bf16 gradient buffer as the loss kernels are handed it: they write zeros into the padding."""
    return _B16.alloc_rows(M, N, device, kernel_zeroes_pad=True)


def _input_grad(fmt, dy, ldy, flags, weight, dims, dres, keep, in_shape, live, as_f32=False):
    """dX = dY W (+ dres), viewed as `in_shape`, for y = x W^T with dims = (M, K, N): dY is [M, N] rows of `fmt` with leading dimension `ldy` and
    GEMM `flags`, W the [N, K] master weight.  `dres` is the gradient of the residual branch that skips the sublayer (or None): the GEMM
    accumulates into it (beta = 1) when `fmt.accumulate_target` allows -- `keep` are the tensors that rule treats as live -- else the product gets
    its own buffer and an add follows; `as_f32` (an fp32 input of the bf16-resident path) then lets the gradient leave as fp32.  `live`: the
    LiveRows of the scope, or None (the launch computes the listed rows only where the list has `perm`)."""
    M, K, N = dims
    w, ldw = fmt.weight(weight)
    acc = fmt.accumulate_target(dres, M, K, *keep)
    if acc is not None:          # dx = d(residual) + dY W, written over the residual branch's gradient
        fmt.gemm(dy, ldy, 0, w, ldw, 0, acc, K, M, K, N, beta=1.0, flags=flags, **_rows_kw(live))
        return acc.view(in_shape)
    dx = fmt.empty(M, K, dy.device)
    fmt.gemm(dy, ldy, 0, w, ldw, 0, dx, K, M, K, N, flags=flags, **_rows_kw(live))
    dx = dx.view(in_shape)
    if dres is not None:
        dx = dx + dres.reshape(in_shape)
    return dx.float() if as_f32 else dx


def _weight_grads(fmt, dy, ldy, flags, x2, ldx, dims, wtargets, btargets, live, want_dw=True, want_db=True):
    """(dW [N, K], db [N]) of y = x W^T + b with dims = (M, N, K), fp32 in either format, each in its gradient-arena slot where it has one
    (`_grad_buffer`); None for the one not wanted.  dW = dY^T X contracts over the rows of `live` (LiveRows or None); db = the column sums of
    dY = the row sums of that launch's A operand rides on it (`rowsum`) and falls back to `colsum` where the launch reports "not done" -- or
    where there is no launch, the bias gradient being the only one wanted."""
    M, N, K = dims
    db = _grad_buffer(btargets, (N,), dy.device) if want_db else None
    dw, db_done = None, False
    if want_dw:
        dw = _grad_buffer(wtargets, (N, K), dy.device)
        db_done = fmt.gemm(dy, ldy, 1, x2, ldx, 0, dw, K, N, K, M, flags=flags, rowsum=db, **_live_kw(live, dy))
    if want_db and not db_done:
        d32, ld32 = fmt.f32_rows(dy, ldy, N)
        colsum(d32, M, N, ld32, out=db)
    return dw, db


class LinearFn(torch.autograd.Function):
    """y = act(x W^T + b)  -- nn.Linear + optional erf-GELU / ReLU epilogue on the GEMM of `fmt` (default: fp32 rows on the fp32 MFMA GEMM, whatever
    the precision mode); act = "swish" is the plain GEMM followed by the elementwise kernel ytvln_act_fwd_* (unfused by design: one extra read and
    write of [M, N]).  On bf16 rows x is a bf16 hidden state (or an fp32 network input, cast once), W the bf16 copy of the fp32 master weight and
    y bf16, or fp32 when `out_fp32` (pooled vectors); dW and db are fp32 in either format and go straight into the gradient arena; db rides on the
    dW launch.

    `passthrough=True` returns (y, x): the second output is x itself, to be used by the RESIDUAL connection that skips the sublayer this
    projection opens (vilbert.py:322-325, 365-368: `LayerNorm(dropout(dense(...)) + input_tensor)`).  The residual branch's gradient then
    arrives here as a second output gradient and the input-gradient GEMM accumulates into that buffer (beta = 1) instead of autograd
    launching a separate elementwise add for the fan-out of x."""

    @staticmethod
    def forward(ctx, x, weight, bias, act, passthrough=False, fmt=_F32, out_fp32=False):
        ctx.set_materialize_grads(False)
        ctx.passthrough, ctx.fmt = bool(passthrough), fmt
        xf = fmt.cast(x)
        ctx.x_was_f32 = xf is not x          # an fp32 input of the bf16-resident path: cast on entry, and its gradient leaves as fp32
        x2, M, K, lda = fmt.rows(xf, "x")
        _check(weight, "weight")
        if weight.stride(-1) != 1:
            weight = weight.contiguous()
        N = weight.shape[0]
        assert weight.shape[1] == K, (weight.shape, K)
        out = _F32 if out_fp32 else fmt          # `out_fp32`: the output leaves the bf16-resident path as fp32
        need_grad = any(ctx.needs_input_grad)
        epi = _ACT[act]
        dev = x.device
        live = _live_for(M, fmt)          # inside a live_rows_scope with `forward` set: the GEMM computes the valid rows, padded rows of y (and z) are zeros
        if epi == ACT_SWISH:          # unfused: the plain GEMM writes the pre-activation z (kept for the backward), then y = z * sigmoid(z)
            z, ldy = fmt.empty(M, N, dev), N
            fmt.gemm(x2, lda, 0, *fmt.weight(weight), 1, z, N, M, N, K, bias=bias, **_rows_kw(live, True))
            y = torch.empty_like(z) if need_grad else z          # nothing to keep without a backward: in place
            call("ytvln_act_fwd_" + fmt.suffix, _ptr(z), _ptr(y), M * N, ACT_SWISH, _stream())
            if out is not fmt:
                y = y.float()
        else:
            if out is _F32 and (epi == EPI_NONE or out is not fmt):
                y, ldy = _F32.alloc_rows(M, N, dev)          # wide odd widths (logits) get a 32-float aligned leading dimension
            else:          # (an fp32 activation output stays dense: the ReLU backward reads it as its aux)
                y, ldy = out.empty(M, N, dev), N
            z = fmt.empty(M, N, dev) if (epi == EPI_GELU and need_grad) else None
            fmt.gemm(x2, lda, 0, *fmt.weight(weight), 1, y, ldy, M, N, K, bias=bias, aux=z, ldaux=N, epi=epi, **_rows_kw(live, True))
        ctx.epi, ctx.dims, ctx.lda, ctx.has_bias = epi, (M, N, K), lda, bias is not None
        ctx.live = live if need_grad else None
        ctx.in_shape = x.shape
        ctx.targets = _targets_of(weight)
        ctx.btargets = _targets_of(bias) if bias is not None else None
        # the ReLU backward needs the sign of the OUTPUT: a bf16 copy of it when the output itself leaves as fp32
        aux = z if epi in (EPI_GELU, ACT_SWISH) else ((y if out is fmt else fmt.cast(y)) if (epi == EPI_RELU and need_grad) else None)
        ctx.save_for_backward(x2, weight, aux)
        out = _view_rows_as(y, ldy, tuple(x.shape[:-1]) + (N,))
        return (out, x) if ctx.passthrough else out

    @staticmethod
    def backward(ctx, dy, dres=None):
        tail = (None,) * (len(ctx.needs_input_grad) - 3)          # act, passthrough, fmt, out_fp32: as many as the call passed
        if dy is None:
            return ((dres if ctx.needs_input_grad[0] else None), None, None) + tail
        fmt = ctx.fmt
        x2, weight, aux = ctx.saved_tensors
        M, N, K = ctx.dims
        dy_in = dy
        dy, ldy, flags = fmt.grad_rows(dy, M, N)
        if ctx.epi != EPI_NONE:
            if ldy != N:
                dy, ldy, flags = dy.contiguous(), N, 0
            dz = fmt.empty(M, N, dy.device)
            call("ytvln_act_bwd_" + fmt.suffix, _ptr(dy), _ptr(aux), _ptr(dz), M * N, ctx.epi, _stream())
            dy = dz
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _input_grad(fmt, dy, ldy, flags, weight, (M, K, N), dres, (dy, dy_in), ctx.in_shape, ctx.live, as_f32=ctx.x_was_f32)
        dw, db = _weight_grads(fmt, dy, ldy, flags, x2, ctx.lda, (M, N, K), ctx.targets, ctx.btargets, ctx.live,
                               want_dw=ctx.needs_input_grad[1], want_db=ctx.has_bias and ctx.needs_input_grad[2])
        return (dx, dw, db) + tail


def _wants_bf16(x: Tensor, weight: Tensor) -> bool:
    """bf16-resident path for this projection?  Yes when its input already is a bf16 hidden state; in bf16 mode also for a LARGE projection
    whose input arrives as fp32 (the 2048-d region features: cast once on the way in)."""
    if x.dtype == torch.bfloat16:
        return True
    K = x.shape[-1]
    return x.dtype == torch.float32 and _bf16_eligible(x.numel() // max(K, 1), weight.shape[0], K)


def linear(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, act: Optional[str] = None, out_fp32: bool = False) -> Tensor:
    """`out_fp32` only matters on the bf16-resident path: the output leaves the path as fp32 (the pooled vectors and the small heads on them)."""
    return LinearFn.apply(x, weight, bias, act, False, _B16 if _wants_bf16(x, weight) else _F32, out_fp32)


def linear_res(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, act: Optional[str] = None) -> Tuple[Tensor, Tensor]:
    """(linear(x, ...), x): use the second value for the residual connection around the sublayer (see LinearFn)."""
    return LinearFn.apply(x, weight, bias, act, True, _B16 if _wants_bf16(x, weight) else _F32)


class FFNFn(torch.autograd.Function):
    """out = gelu(x W1^T + b1) W2^T + b2   (BertIntermediate + BertOutput.dense, vilbert.py:351-354, 365).
    Backward fuses the GELU derivative into the epilogue of the dX GEMM of the second projection.  x, the GELU pre-activation z, the hidden h and
    out are rows of `fmt`; weight and bias gradients are fp32.

    `recompute_h=True` (BertEncoder.recompute = "ffn"; fp32 rows only, see `ffn`): the node keeps the pre-activation z and not h = gelu(z) -- M x I x 4 bytes less per FFN
    between forward and backward -- and its backward rebuilds h with ytvln_gelu_fwd_f32 (the epilogue's own device function on the stored z:
    the same bits) into a buffer that lives from just before the dW2 GEMM to just after it.  Everything else is the default path."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, passthrough=False, recompute_h=False, fmt=_F32):
        ctx.set_materialize_grads(False)
        ctx.passthrough, ctx.fmt = bool(passthrough), fmt
        ctx.recompute_h = bool(recompute_h)
        x2, M, K, lda = fmt.rows(x, "x")
        I, N = w1.shape[0], w2.shape[0]
        need_grad = any(ctx.needs_input_grad)
        dev = x.device
        h = fmt.empty(M, I, dev)
        z = fmt.empty(M, I, dev) if need_grad else None
        live = _live_for(M, fmt)
        fmt.gemm(x2, lda, 0, *fmt.weight(w1), 1, h, I, M, I, K, bias=b1, aux=z, ldaux=I, epi=EPI_GELU, **_rows_kw(live, True))
        y = fmt.empty(M, N, dev)
        fmt.gemm(h, I, 0, *fmt.weight(w2), 1, y, N, M, N, I, bias=b2, **_rows_kw(live, True))
        ctx.dims, ctx.lda, ctx.in_shape = (M, K, I, N), lda, x.shape
        ctx.live = live if need_grad else None
        ctx.targets = (_targets_of(w1), _targets_of(w2), _targets_of(b1), _targets_of(b2))
        ctx.save_for_backward(x2, w1, w2, z, None if ctx.recompute_h else h)
        out = y.view(*x.shape[:-1], N)
        return (out, x) if ctx.passthrough else out

    @staticmethod
    def backward(ctx, dy, dres=None):
        tail = (None,) * (len(ctx.needs_input_grad) - 5)          # passthrough / recompute_h / fmt: as many as the call passed
        if dy is None:
            return ((dres if ctx.needs_input_grad[0] else None), None, None, None, None) + tail
        fmt = ctx.fmt
        x2, w1, w2, z, h = ctx.saved_tensors
        M, K, I, N = ctx.dims
        dy_in = dy
        dy, ldy, _ = fmt.grad_rows(dy, M, N)
        dev = dy.device
        dz = fmt.empty(M, I, dev)
        fmt.gemm(dy, ldy, 0, *fmt.weight(w2), 0, dz, I, M, I, N, aux=z, ldaux=I, epi=EPI_MUL_DGELU, **_rows_kw(ctx.live))   # dH * gelu'(z)
        if h is None:          # recompute_h: h = gelu(z), alive for the one GEMM that reads it
            h = fmt.empty(M, I, dev)
            call("ytvln_gelu_fwd_f32", _ptr(z), _ptr(h), M * I, _stream())
        dw2, db2 = _weight_grads(fmt, dy, ldy, 0, h, I, (M, N, I), ctx.targets[1], ctx.targets[3], ctx.live)          # db2 rides on the dW2 GEMM
        del h
        dx = None
        if ctx.needs_input_grad[0]:          # the residual around the FFN: accumulated into its gradient where possible (see LinearFn)
            # (dy is consumed by now, but it may be retained / hooked upstream)
            dx = _input_grad(fmt, dz, I, 0, w1, (M, K, I), dres, (dy, dy_in), ctx.in_shape, ctx.live)
        dw1, db1 = _weight_grads(fmt, dz, I, 0, x2, ctx.lda, (M, I, K), ctx.targets[0], ctx.targets[2], ctx.live)
        return (dx, dw1, db1, dw2, db2) + tail


_NO_BF16_RECOMPUTE_H = ('recompute = "ffn" with bf16 hidden states: the bf16-resident path stores the GELU pre-activation z rounded to bf16, and '
                        'bf16(gelu(float(bf16 z))) is not the stored h -- the tier would not be exact.  Use recompute = "layer" (exact on this '
                        'path) or "none"')


def _ffn(x, w1, b1, w2, b2, passthrough: bool, recompute_h: bool):
    fmt = _format_of(x)
    if recompute_h and not fmt.exact_gelu_replay:
        raise NotImplementedError(_NO_BF16_RECOMPUTE_H)
    return FFNFn.apply(x, w1, b1, w2, b2, passthrough, recompute_h, fmt)


def ffn(x, w1, b1, w2, b2, recompute_h: bool = False) -> Tensor:
    """`recompute_h`: see FFNFn (fp32 hidden states only; bf16 ones are refused)."""
    return _ffn(x, w1, b1, w2, b2, False, recompute_h)


def ffn_res(x, w1, b1, w2, b2, recompute_h: bool = False) -> Tuple[Tensor, Tensor]:
    """(ffn(x, ...), x) -- the second value feeds the residual add behind the FFN (see LinearFn)."""
    return _ffn(x, w1, b1, w2, b2, True, recompute_h)


# ------------------------------------------------------------------------------------------------------------------
# bf16-resident path (BASELINE configs[4]; set_matmul_precision("bf16")): hidden states, their gradients and a copy of the weights
# are bf16 tensors in HBM; ytvln_gemm_bf16 / ytvln_attn_*_bf16 / ytvln_ln_*_bf16 read and write them in place.  No operand is
# staged, cast or transposed per call: the producer of a tensor writes the bf16 its consumers read.
# ------------------------------------------------------------------------------------------------------------------
_BF16 = torch.bfloat16
_BF16_WS_CACHE = {}
_DT_CODE = {torch.float32: _lib.DT_F32, torch.bfloat16: _lib.DT_BF16}


def _pad8(n: int) -> int:
    """Leading dimension (elements) of a bf16 row buffer whose width is not a multiple of 8: rounded up to 64, the padding ZERO."""
    return n if n % 8 == 0 else (n + 63) // 64 * 64


def cast_bf16(x: Tensor) -> Tensor:
    """bf16 copy (round to nearest even) of a contiguous fp32 tensor: network inputs entering the bf16-resident path, parameters outside the
    optimizer's arenas, small fp32 gradients coming back from the fp32 heads."""
    _check(x, "x")
    xc = x if x.is_contiguous() else x.contiguous()
    out = torch.empty(xc.shape, dtype=_BF16, device=x.device)
    cols = xc.shape[-1] if xc.dim() > 1 else xc.numel()
    rows = xc.numel() // max(cols, 1)
    if xc.numel():
        call("ytvln_cast_f32_bf16", _ptr(xc), cols, rows, cols, out.data_ptr(), cols, _stream())
    return out


def _bf16_weight(weight: Tensor) -> Tensor:
    """The bf16 copy of a weight operand ([out, in], contiguous).  Parameters that live in the optimizer's flat arena (after the first
    optimizer step: all that receive gradients) have their copy in a bf16 arena at the same offsets, refreshed by the AdamW kernel itself
    (ytvln_adamw_f32_bf16copy) -- a packed Q|K|V operand is then a zero-copy view of it.  Everything else (the first eager steps, frozen
    or inference-only parameters) is cast on the spot and cached against the parameter's version counter."""
    targets = _targets_of(weight)
    if targets:
        first = _slot_of(targets[0])
        if first is not None and first.owner is not None:
            off, ok = first.off, True
            for t in targets:
                sl = _slot_of(t)
                if sl is None or sl.flat_p is not first.flat_p or sl.off != off:
                    ok = False
                    break
                off += sl.numel
            opt = first.owner() if ok else None
            if opt is not None:
                pb = opt.bf16_arena(targets)
                if pb is not None:
                    return pb[first.off:off].view(weight.shape)
        # not (all) adjacent in one arena.  Arena members are updated by the fused AdamW kernel through raw pointers, which does not bump
        # their version counters: a cache keyed on versions would go stale after every optimizer step, so they are cast on the spot.
        if any(_slot_of(t) is not None for t in targets):
            return cast_bf16(weight.detach())
        # per-parameter cache keyed by (storage pointer, version)
        key = tuple((t.data_ptr(), t._version) for t in targets)
        holder = targets[0]
        cached = getattr(holder, "_ytvln_bf16_cache", None)
        if cached is not None and cached[0] == key and cached[1].shape == weight.shape:
            return cached[1]
        wb = cast_bf16(weight.detach())
        if not torch.cuda.is_current_stream_capturing():
            holder._ytvln_bf16_cache = (key, wb)
        return wb
    return cast_bf16(weight.detach())


def _gemm_bf16(A, lda, transA, B, ldb, transB, C, ldc, M, N, K, bias=None, aux=None, ldaux=0, epi=EPI_NONE, beta=0.0, flags=0, rowsum=None):
    """ytvln_gemm_bf16: bf16 operands read in place (transA = 1 / transB = 0: the contraction index is the operand's ROW, gathered by the
    transposing LDS read), fp32 accumulation, C bf16 or fp32.  Returns True when `rowsum` ([M] fp32: sum_k op(A)[m, k]) was produced."""
    key = (M, N, K, epi)
    need = _BF16_WS_CACHE.get(key)
    if need is None:
        need = _BF16_WS_CACHE[key] = int(_lib.load().ytvln_gemm_bf16_workspace_elems(M, N, K, epi))
    ws = torch.empty(need, dtype=torch.float32, device=C.device) if need else None
    done = ctypes.c_int(0)
    call("ytvln_gemm_bf16", A.data_ptr(), lda, int(transA), B.data_ptr(), ldb, int(transB), C.data_ptr(), ldc, _DT_CODE[C.dtype], _ptr(bias),
         aux.data_ptr() if aux is not None else None, ldaux, M, N, K, epi, float(beta), _ptr(ws), need, int(flags),
         _ptr(rowsum) if rowsum is not None else None, ctypes.byref(done) if rowsum is not None else None, _stream())
    return bool(done.value)


# ------------------------------------------------------------------------------------------------------------------
# LayerNorm family
# ------------------------------------------------------------------------------------------------------------------
def _ln_bwd(dy, s, mean, rstd, gamma, rows, H, p_pre, p_post, rng, site, gb_targets=None, fmt=_F32, want_rows=True, want_f32=False):
    """-> (ds, dx (= ds when p_pre == 0), dgamma, dbeta), ds / dx rows of `fmt`; statistics, gamma / beta and their gradients fp32.
    `want_f32` (the embedding-table gradient kernels read fp32 rows) -> (ds | None, dx, ds as fp32 rows, dgamma, dbeta): fp32 rows serve as they
    are, bf16 rows get an fp32 copy written by the same launch, and the bf16 ds itself only with `want_rows`."""
    dy = fmt.cast(dy.reshape(rows, H)).reshape(rows, H)
    if not dy.is_contiguous():
        dy = dy.contiguous()
    dev = dy.device
    copy32 = want_f32 and fmt.ln_bwd_f32_copy
    ds = fmt.empty(rows, H, dev) if (want_rows or not copy32) else None
    dx = fmt.empty(rows, H, dev) if p_pre > 0 else None
    ds32 = torch.empty((rows, H), dtype=torch.float32, device=dev) if copy32 else None
    nb = _lib.load().ytvln_ln_bwd_blocks(rows)
    partial = torch.empty((nb, 2 * H), dtype=torch.float32, device=dev)
    call("ytvln_ln_bwd_" + fmt.suffix, _ptr(dy), _ptr(s), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(ds), _ptr(dx),
         *((_ptr(ds32),) if fmt.ln_bwd_f32_copy else ()), _ptr(partial), rows, H, float(p_pre), float(p_post),
         _ptr(rng) if rng is not None else None, int(site), _stream())
    gb = colsum(partial, nb, 2 * H, 2 * H, out=_direct_grad(gb_targets, (2 * H,)))      # LayerNorm.weight | LayerNorm.bias
    dx = dx if dx is not None else ds
    if want_f32:
        return ds, dx, (ds32 if copy32 else ds), gb[:H], gb[H:]
    return ds, dx, gb[:H], gb[H:]


def _one_sided_dropout(p_pre, p_post) -> None:
    """The row kernels draw the dropout in front of the LayerNorm and the one behind it from the same (key, site, row, vector) bits: asked for both,
    the two masks would be fully correlated (identical at p_pre == p_post).  No site of the model uses both, so the combination is refused here and
    again at the C ABI."""
    if p_pre > 0 and p_post > 0:
        raise RuntimeError(f"add_layer_norm: p_pre = {p_pre} and p_post = {p_post} are both > 0; one call draws one mask -- use p_pre or p_post "
                           "and a separate ops.dropout for the other")


class AddLayerNormFn(torch.autograd.Function):
    """y = LN(dropout(x) + residual) [dropout after] -- BertLayerNorm with its surrounding dropout / residual add, on rows of `fmt` (statistics,
    gamma / beta and their gradients fp32); saves s = dropout(x) + residual in that format.  At most one of p_pre / p_post may be > 0."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta, eps, p_pre, p_post, rng, site, fmt=_F32):
        ctx.set_materialize_grads(False)
        ctx.fmt = fmt
        _one_sided_dropout(p_pre, p_post)
        _check(x, "x", fmt.dtype)
        H = x.shape[-1]
        xc = x if x.is_contiguous() else x.contiguous()
        rc = None
        if res is not None:
            _check(res, "residual", fmt.dtype)
            rc = res if res.is_contiguous() else res.contiguous()
        rows = xc.numel() // H
        need_grad = any(ctx.needs_input_grad)
        y = torch.empty_like(xc)
        s = torch.empty_like(xc) if need_grad else None
        mean = torch.empty(rows, dtype=torch.float32, device=x.device) if need_grad else None
        rstd = torch.empty_like(mean) if need_grad else None
        call("ytvln_ln_fwd_" + fmt.suffix, _ptr(xc), _ptr(rc), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(s), _ptr(mean), _ptr(rstd), rows, H,
             float(eps), float(p_pre), float(p_post), _ptr(rng) if rng is not None else None, int(site), _stream())
        ctx.meta = (rows, H, p_pre, p_post, site, res is not None)
        ctx.gb = (gamma, beta) if isinstance(gamma, torch.nn.Parameter) and isinstance(beta, torch.nn.Parameter) else None
        ctx.save_for_backward(s, mean, rstd, gamma, rng)
        return y

    @staticmethod
    def backward(ctx, dy):
        tail = (None,) * (len(ctx.needs_input_grad) - 4)
        if dy is None:
            return (None,) * 4 + tail
        s, mean, rstd, gamma, rng = ctx.saved_tensors
        rows, H, p_pre, p_post, site, has_res = ctx.meta
        ds, dx, dg, db = _ln_bwd(dy, s, mean, rstd, gamma, rows, H, p_pre, p_post, rng, site, ctx.gb, ctx.fmt)
        shape = dy.shape
        return (dx.view(shape) if ctx.needs_input_grad[0] else None,
                ds.view(shape) if (has_res and ctx.needs_input_grad[1]) else None, dg, db) + tail


def add_layer_norm(x, res, gamma, beta, eps=1e-12, p_pre=0.0, p_post=0.0, drop: Optional[DropoutState] = None) -> Tensor:
    if (p_pre > 0 or p_post > 0) and drop is None:
        raise RuntimeError("dropout requested without a DropoutState")
    _one_sided_dropout(p_pre, p_post)
    use = drop is not None and (p_pre > 0 or p_post > 0)
    return AddLayerNormFn.apply(x, res, gamma, beta, eps, p_pre if use else 0.0, p_post if use else 0.0,
                                drop.tensor if use else None, drop.next_site() if use else 0, _format_of(x))


class TextEmbedFn(torch.autograd.Function):
    """BertEmbeddings.forward (vilbert.py:240-256) fused: gather x3 + add + LayerNorm + dropout."""

    @staticmethod
    def forward(ctx, ids, type_ids, word, pos, typ, gamma, beta, eps, p_post, rng, site):
        ctx.set_materialize_grads(False)
        ids = _i64(ids, "input_ids")
        N, T = ids.shape
        H = word.shape[1]
        if T > pos.shape[0]:
            raise RuntimeError(f"sequence length {T} exceeds max_position_embeddings {pos.shape[0]}")
        tt = _i64(type_ids, "token_type_ids") if type_ids is not None else None
        rows = N * T
        need_grad = any(ctx.needs_input_grad)
        bf16 = _MATMUL_PRECISION == "bf16"          # bf16-resident path: the hidden states leave the embedding as bf16
        y = torch.empty((N, T, H), dtype=torch.bfloat16 if bf16 else torch.float32, device=word.device)
        s = torch.empty_like(y) if need_grad else None
        mean = torch.empty(rows, dtype=torch.float32, device=word.device) if need_grad else None
        rstd = torch.empty_like(mean) if need_grad else None
        call("ytvln_text_embed_fwd_bf16" if bf16 else "ytvln_text_embed_fwd_f32", _ptr(ids), _ptr(tt), _ptr(word), _ptr(pos), _ptr(typ),
             _ptr(gamma), _ptr(beta), _ptr(y), _ptr(s), _ptr(mean), _ptr(rstd), rows, T, H, float(eps), float(p_post),
             _ptr(rng) if rng is not None else None, int(site), _stream())
        ctx.meta = (N, T, H, p_post, site, word.shape, pos.shape, typ.shape)
        ctx.save_for_backward(ids, tt, s, mean, rstd, gamma, rng)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return (None,) * 11
        ids, tt, s, mean, rstd, gamma, rng = ctx.saved_tensors
        N, T, H, p_post, site, wshape, pshape, tshape = ctx.meta
        rows = N * T
        # the table-gradient kernels below read fp32 rows of ds (bf16-resident path: an fp32 copy, and no bf16 ds: nothing reads it)
        _, _, ds, dg, db = _ln_bwd(dy, s, mean, rstd, gamma, rows, H, 0.0, p_post, rng, site, fmt=_format_of(s), want_rows=False, want_f32=True)
        dev = ds.device
        dword = torch.zeros(wshape, dtype=torch.float32, device=dev)
        # token ids repeat inside a batch: sorted (stable) so that one wave owns each id's run -- no atomics, reproducible sums
        sorted_ids, perm = torch.sort(ids.reshape(-1), stable=True)
        call("ytvln_scatter_add_rows_sorted_f32", _ptr(ds), H, _ptr(sorted_ids), _ptr(perm), rows, H, _ptr(dword), 0, _stream())   # padding_idx = 0
        dpos = torch.zeros(pshape, dtype=torch.float32, device=dev)
        dpos[:T] = colsum(ds, N, T * H, T * H).view(T, H)
        if tt is None:
            dtyp = torch.zeros(tshape, dtype=torch.float32, device=dev)
            dtyp[0] = colsum(ds, rows, H, H)
        elif tshape[0] <= 32:
            dtyp = colsum_by_index(ds, rows, H, H, tshape[0], idx_i64=tt)
        else:
            dtyp = torch.zeros(tshape, dtype=torch.float32, device=dev)
            call("ytvln_scatter_add_rows_f32", _ptr(ds), H, _ptr(tt), rows, H, _ptr(dtyp), -1, _stream())
        return None, None, dword, dpos, dtyp, dg, db, None, None, None, None


_CHECK_INDICES = os.environ.get("YTVLN_CHECK_INDICES", "0") != "0"


def _check_index_range(idx: Tensor, n: int, what: str) -> None:
    """Debug aid (YTVLN_CHECK_INDICES=1; one host sync per call): the embedding kernels gather rows by raw index like torch's own
    kernels, which assert on the device; production keeps the sync-free path."""
    if _CHECK_INDICES and idx.numel():
        lo, hi = int(idx.min()), int(idx.max())
        if lo < 0 or hi >= n:
            raise IndexError(f"{what}: index range [{lo}, {hi}] outside the table of {n} rows")


def text_embed(ids, type_ids, word, pos, typ, gamma, beta, eps=1e-12, p=0.0, drop: Optional[DropoutState] = None) -> Tensor:
    _check_index_range(ids, word.shape[0], "token ids")
    if type_ids is not None:
        _check_index_range(type_ids, typ.shape[0], "token type ids")
    use = drop is not None and p > 0
    return TextEmbedFn.apply(ids, type_ids, word, pos, typ, gamma, beta, eps, p if use else 0.0, drop.tensor if use else None,
                             drop.next_site() if use else 0)


class ImageEmbedFn(torch.autograd.Function):
    """BertImageEmbeddings.forward after the feature projection (vilbert.py:1361-1368), fused:
    location / orientation / next-orientation linears (K = 5, 4, 2) + frame-index gather + add + LayerNorm + dropout."""

    @staticmethod
    def forward(ctx, img, loc, W5, b5, W4, b4, W2, b2, E, gamma, beta, eps, p_post, rng, site):
        ctx.set_materialize_grads(False)
        bf16 = img.dtype == torch.bfloat16          # bf16-resident path: img is the bf16 output of the feature projection
        _check(img, "img", img.dtype if bf16 else torch.float32)
        _check(loc, "image_loc")
        H = img.shape[-1]
        imgc = img if img.is_contiguous() else img.contiguous()
        locc = loc if loc.is_contiguous() else loc.contiguous()
        if locc.shape[-1] != 12:
            raise RuntimeError(f"image_loc must have 12 columns (5 box + 4 orientation + 2 next-orientation + frame); got {locc.shape}")
        rows = imgc.numel() // H
        need_grad = any(ctx.needs_input_grad)
        y = torch.empty_like(imgc)
        s = torch.empty_like(imgc) if need_grad else None
        mean = torch.empty(rows, dtype=torch.float32, device=img.device) if need_grad else None
        rstd = torch.empty_like(mean) if need_grad else None
        ws = [w if w.is_contiguous() else w.contiguous() for w in (W5, W4, W2, E)]
        call("ytvln_image_embed_fwd_bf16" if bf16 else "ytvln_image_embed_fwd_f32", _ptr(imgc), _ptr(locc), _ptr(ws[0]), _ptr(b5), _ptr(ws[1]), _ptr(b4), _ptr(ws[2]), _ptr(b2),
             _ptr(ws[3]), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(s), _ptr(mean), _ptr(rstd), rows, H, float(eps), float(p_post),
             _ptr(rng) if rng is not None else None, int(site), _stream())
        ctx.meta = (rows, H, p_post, site, E.shape[0])
        ctx.live = _live_for(rows, _F32 if not bf16 else None) if need_grad else None
        ctx.save_for_backward(locc, s, mean, rstd, gamma, rng)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return (None,) * 15
        locc, s, mean, rstd, gamma, rng = ctx.saved_tensors
        rows, H, p_post, site, KT = ctx.meta
        # ds in img's format for the feature projection's backward, as fp32 rows for the small kernels below (fp32 path: one and the same buffer)
        dimg, _, ds, dg, db = _ln_bwd(dy, s, mean, rstd, gamma, rows, H, 0.0, p_post, rng, site, fmt=_format_of(s), want_f32=True)
        dev = ds.device
        dwall = torch.empty((H, 12), dtype=torch.float32, device=dev)
        _gemm(ds, H, 1, locc, 12, 0, dwall, 12, H, 12, rows, **_live_kw(ctx.live, ds))               # ds^T . loc  -> [H, 12]
        dbias = colsum(ds, rows, H, H)
        dE = colsum_by_index(ds, rows, H, H, KT, idx_f32=locc, idx_stride=12, idx_f32_offset=11)
        return (dimg.view(dy.shape), None, dwall[:, 0:5].contiguous(), dbias, dwall[:, 5:9].contiguous(), dbias,
                dwall[:, 9:11].contiguous(), dbias, dE, dg, db, None, None, None, None)


def image_embed(img, loc, W5, b5, W4, b4, W2, b2, E, gamma, beta, eps=1e-12, p=0.0, drop: Optional[DropoutState] = None) -> Tensor:
    if _CHECK_INDICES:
        _check_index_range(loc[..., 11].long(), E.shape[0], "frame index (image_loc[..., 11])")
    use = drop is not None and p > 0
    if _MATMUL_PRECISION == "bf16" and img.dtype == torch.float32:
        # both streams of the bf16-resident path are bf16 (co-attention reads them side by side); a feature projection too small for the bf16
        # GEMM (K < 64: toy configs) leaves its output fp32 -- round it here, autograd casts the gradient back
        img = img.to(torch.bfloat16)
    return ImageEmbedFn.apply(img, loc, W5, b5, W4, b4, W2, b2, E, gamma, beta, eps, p if use else 0.0,
                              drop.tensor if use else None, drop.next_site() if use else 0)


class GatherRowsFn(torch.autograd.Function):
    """out[j] = x[idx[j]] over rows of a [M, H] matrix (idx < 0 -> zero row); backward scatters the row gradients back."""

    @staticmethod
    def forward(ctx, x, idx):
        ctx.set_materialize_grads(False)
        x2, M, H, ld = _F32.rows(x, "x")
        idx = _i64(idx, "idx").reshape(-1)
        out = torch.empty((idx.numel(), H), dtype=torch.float32, device=x.device)
        call("ytvln_gather_rows_f32", _ptr(x2), ld, _ptr(idx), idx.numel(), H, _ptr(out), _stream())
        ctx.meta = (M, H, x.shape)
        ctx.save_for_backward(idx)
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None
        (idx,) = ctx.saved_tensors
        M, H, shape = ctx.meta
        g = g if g.is_contiguous() else g.contiguous()
        dx = torch.zeros((M, H), dtype=torch.float32, device=g.device)
        call("ytvln_scatter_add_rows_f32", _ptr(g), H, _ptr(idx), idx.numel(), H, _ptr(dx), -1, _stream())
        return dx.view(shape), None


def gather_rows(x: Tensor, idx: Tensor) -> Tensor:
    return GatherRowsFn.apply(x, idx)


def select_rows(flag: Tensor, capacity: int) -> Tensor:
    """Static-shape, sync-free row selection: the first `capacity` indices of a stable sort that puts flagged rows first.
    If fewer rows are flagged the tail holds un-flagged rows (their targets are "ignore", so they change no loss); callers
    size `capacity` well above the expected count and may check `flag.sum() <= capacity` lazily."""
    order = torch.argsort((~flag.reshape(-1).bool()).to(torch.int8), stable=True)
    return order[:capacity].contiguous()


# ------------------------------------------------------------------------------------------------------------------
# packed rows (BertModel.skip_padding): the valid rows of a padded batch, moved by one kernel in all four directions
# ------------------------------------------------------------------------------------------------------------------
class RowsPlan:
    """ytvln_rows_plan's outputs for one padding mask: `pack_idx` [capacity] (padded row of each packed row, -1 past the count), `unpack_idx`
    [rows] (packed row of each padded row, -1 where there is none), `counts` [2] (flagged rows, flagged rows that did not fit) -- device int64
    tensors -- and the two host integers `rows` and `capacity`."""
    __slots__ = ("pack_idx", "unpack_idx", "counts", "rows", "capacity")

    def __init__(self, pack_idx, unpack_idx, counts, rows, capacity):
        self.pack_idx, self.unpack_idx, self.counts, self.rows, self.capacity = pack_idx, unpack_idx, counts, int(rows), int(capacity)

    def record_stream(self, stream) -> None:
        for t in (self.pack_idx, self.unpack_idx, self.counts):
            t.record_stream(stream)


def rows_capacity(rows: int, frac: float) -> int:
    """Static capacity of a side: min(rows, ceil(frac * rows / 256) * 256) -- whole 256-row GEMM tiles, never more than the padded rows."""
    return min(int(rows), int(math.ceil(float(frac) * int(rows) / 256.0)) * 256)


def rows_plan(mask: Tensor, capacity: int) -> RowsPlan:
    """Plan of the rows of `mask` (any shape; non-zero = valid) with room for `capacity` packed rows.  One launch, no host sync."""
    if not mask.is_cuda:
        raise RuntimeError(f"ytvln.ops: `mask` must live on the GPU (no CPU fallback); got device {mask.device}")
    rows, capacity = mask.numel(), int(capacity)
    flags = (mask.reshape(-1) != 0).contiguous()          # one byte per row
    pack_idx = torch.empty(max(capacity, 0), dtype=torch.int64, device=mask.device)
    unpack_idx = torch.empty(rows, dtype=torch.int64, device=mask.device)
    counts = torch.empty(2, dtype=torch.int64, device=mask.device)
    call("ytvln_rows_plan", flags.data_ptr(), rows, capacity, pack_idx.data_ptr(), unpack_idx.data_ptr(), counts.data_ptr(), _stream())
    return RowsPlan(pack_idx, unpack_idx, counts, rows, capacity)


def _rows_move(x2: Tensor, ld: int, x_rows: int, idx: Tensor, out_rows: int, width: int) -> Tensor:
    out = torch.empty((out_rows, width), dtype=x2.dtype, device=x2.device)
    call("ytvln_rows_move_bf16" if x2.dtype == torch.bfloat16 else "ytvln_rows_move_f32", x2.data_ptr(), ld, x_rows, idx.data_ptr(), out_rows, width,
         out.data_ptr(), width, _stream())
    return out


class RowsMoveFn(torch.autograd.Function):
    """out[j] = x[idx[j]] (zero rows where idx[j] < 0) over the rows of a [M, W] matrix, fp32 or bf16, read through (pointer, leading dimension).
    `back_idx` is the other index array of the same plan: the backward is the same kernel with it."""

    @staticmethod
    def forward(ctx, x, idx, out_rows, back_idx):
        ctx.set_materialize_grads(False)
        _check(x, "x", torch.bfloat16 if x.dtype == torch.bfloat16 else torch.float32)
        W = x.shape[-1]
        if x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= W:
            x2, ld = x, x.stride(0)          # a column window / padded leading dimension: read in place
        else:
            x2 = x.reshape(-1, W)
            x2 = x2 if x2.is_contiguous() else x2.contiguous()
            ld = W
        M = x2.shape[0]
        if back_idx.numel() != M or idx.numel() != out_rows:
            raise RuntimeError(f"ytvln.ops: rows of x ({M}) / of the output ({out_rows}) do not match the plan ({back_idx.numel()}, {idx.numel()})")
        ctx.meta = (M, W, x.shape)
        ctx.save_for_backward(back_idx)
        return _rows_move(x2, ld, M, idx, out_rows, W)

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None
        (back_idx,) = ctx.saved_tensors
        M, W, shape = ctx.meta
        g = g if g.is_contiguous() else g.contiguous()
        return _rows_move(g, W, g.shape[0], back_idx, M, W).view(shape), None, None, None


def rows_pack(x: Tensor, plan: RowsPlan) -> Tensor:
    """[capacity, W]: the valid rows of x (`plan.rows` rows of width W, any leading shape) in ascending order, zero rows past the count."""
    return RowsMoveFn.apply(x, plan.pack_idx, plan.capacity, plan.unpack_idx)


def rows_unpack(x: Tensor, plan: RowsPlan) -> Tensor:
    """[rows, W]: packed rows back at their padded places, exact zeros everywhere else."""
    return RowsMoveFn.apply(x, plan.unpack_idx, plan.rows, plan.pack_idx)


class DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, rng, site):
        ctx.set_materialize_grads(False)
        _check(x, "x")
        xc = x if x.is_contiguous() else x.contiguous()
        y = torch.empty_like(xc)
        call("ytvln_dropout_f32", _ptr(xc), _ptr(y), xc.numel(), float(p), _ptr(rng), int(site), _stream())
        ctx.p, ctx.site = p, site
        ctx.save_for_backward(rng)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return None, None, None, None
        (rng,) = ctx.saved_tensors
        dyc = dy if dy.is_contiguous() else dy.contiguous()
        dx = torch.empty_like(dyc)
        call("ytvln_dropout_f32", _ptr(dyc), _ptr(dx), dyc.numel(), float(ctx.p), _ptr(rng), int(ctx.site), _stream())
        return dx, None, None, None


def dropout(x: Tensor, p: float, training: bool, drop: Optional[DropoutState]) -> Tensor:
    if not training or p <= 0.0:
        return x
    if drop is None:
        raise RuntimeError("dropout requested without a DropoutState")
    return DropoutFn.apply(x, p, drop.tensor, drop.next_site())


# ------------------------------------------------------------------------------------------------------------------
# heads of the downstream-task model (vilbert.py:1457-1535): weight normalisation over a whole matrix, one-feature Linear over rows
# ------------------------------------------------------------------------------------------------------------------
class WeightNormFn(torch.autograd.Function):
    """w = v * g / ||v||_F with one scalar g per matrix (torch.nn.utils.weight_norm(..., dim=None), vilbert.py:1526-1529).  The backward takes
    dL/dw from the projection that consumed w and writes dv / dg straight into the gradient arena when the two parameters live there."""

    @staticmethod
    def forward(ctx, v, g):
        ctx.set_materialize_grads(False)
        _check(v, "weight_v")
        _check(g, "weight_g")
        if g.numel() != 1:
            raise RuntimeError(f"ytvln.ops.weight_norm: weight_g must hold one element (dim=None); got shape {tuple(g.shape)}")
        vc = v if v.is_contiguous() else v.contiguous()
        n = vc.numel()
        w = torch.empty_like(vc)
        stat = torch.empty(2, dtype=torch.float32, device=v.device)
        ws = torch.empty(_lib.load().ytvln_weight_norm_workspace_elems(n), dtype=torch.float32, device=v.device)
        # no bf16 copy of w (the kernel can write one): the only consumer, SimpleClassifier, feeds the fp32 GEMM in every precision mode
        call("ytvln_weight_norm_fwd_f32", _ptr(vc), _ptr(g), n, _ptr(w), None, _ptr(stat), _ptr(ws), _stream())
        ctx.vtargets, ctx.gtargets = _targets_of(v), _targets_of(g)
        ctx.save_for_backward(vc, stat)
        return w

    @staticmethod
    def backward(ctx, dw):
        if dw is None:
            return None, None
        vc, stat = ctx.saved_tensors
        dwc = dw if dw.is_contiguous() else dw.contiguous()
        n = vc.numel()
        dv = _direct_grad(ctx.vtargets, vc.shape)
        if dv is None:
            dv = torch.empty_like(vc)
        dg = _direct_grad(ctx.gtargets, ())
        if dg is None:
            dg = torch.empty((), dtype=torch.float32, device=vc.device)
        ws = torch.empty(_lib.load().ytvln_weight_norm_workspace_elems(n), dtype=torch.float32, device=vc.device)
        call("ytvln_weight_norm_bwd_f32", _ptr(vc), _ptr(dwc), _ptr(stat), n, _ptr(dv), _ptr(dg), _ptr(ws), _stream())
        return dv, dg


def weight_norm(v: Tensor, g: Tensor) -> Tensor:
    """The effective weight of a weight-normed Linear: pass it to `linear` like any [out, in] weight."""
    return WeightNormFn.apply(v, g)


class RowLogitFn(torch.autograd.Function):
    """out[..., 0] = (dropout(x) . w + b) + (1 - mask) * -10000: nn.Linear(H, 1) over every row of an fp32 or bf16 hidden state, fused with the
    dropout in front of it and the region-mask term behind it (vilbert.py:1517-1518).  The output is fp32; dx has x's type."""

    @staticmethod
    def forward(ctx, x, weight, bias, mask, p, rng, site):
        ctx.set_materialize_grads(False)
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise RuntimeError(f"ytvln.ops.row_logit: `x` must be float32 or bfloat16; got {x.dtype}")
        x2, rows, H, ldx = _format_of(x).rows(x, "x")
        _check(weight, "weight")
        if weight.numel() != H:
            raise RuntimeError(f"ytvln.ops.row_logit: weight of {weight.numel()} elements for rows of {H}")
        ctx.wtargets, ctx.btargets = _targets_of(weight), (_targets_of(bias) if bias is not None else None)
        weight = weight if weight.is_contiguous() else weight.contiguous()
        if bias is not None:
            _check(bias, "bias")
        if mask is not None:
            if mask.numel() != rows:
                raise RuntimeError(f"ytvln.ops.row_logit: mask of {mask.numel()} elements for {rows} rows")
            if mask.dtype != torch.float32 or not mask.is_contiguous():          # (an integer mask: one small cast; an fp32 one is read in place)
                mask = mask.to(torch.float32).contiguous()
            _check(mask, "mask")
        ctx.kind = "bf16" if x.dtype == torch.bfloat16 else "f32"
        out = torch.empty(rows, dtype=torch.float32, device=x.device)
        call("ytvln_row_logit_fwd_" + ctx.kind, x2.data_ptr(), ldx, _ptr(weight), _ptr(bias), _ptr(mask), _ptr(out), rows, H, float(p),
             _ptr(rng), int(site), _stream())
        ctx.dims, ctx.p, ctx.site, ctx.in_shape = (rows, H, ldx), float(p), int(site), x.shape
        ctx.wshape, ctx.has_bias = weight.shape, bias is not None
        ctx.save_for_backward(x2, weight, rng)
        return out.view(tuple(x.shape[:-1]) + (1,))

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return (None,) * 7
        x2, weight, rng = ctx.saved_tensors
        rows, H, ldx = ctx.dims
        dyc = dy.reshape(rows)
        if dyc.dtype != torch.float32 or not dyc.is_contiguous():
            dyc = dyc.to(torch.float32).contiguous()
        dx = torch.empty((rows, H), dtype=x2.dtype, device=x2.device) if ctx.needs_input_grad[0] else None
        dw = _direct_grad(ctx.wtargets, ctx.wshape)
        if dw is None:
            dw = torch.empty(ctx.wshape, dtype=torch.float32, device=x2.device)
        db = None
        if ctx.has_bias:
            db = _direct_grad(ctx.btargets, (1,))
            if db is None:
                db = torch.empty(1, dtype=torch.float32, device=x2.device)
        ws = torch.empty(_lib.load().ytvln_row_logit_workspace_elems(rows, H), dtype=torch.float32, device=x2.device)
        call("ytvln_row_logit_bwd_" + ctx.kind, x2.data_ptr(), ldx, _ptr(weight), _ptr(dyc), rows, H, ctx.p, _ptr(rng), ctx.site,
             dx.data_ptr() if dx is not None else None, H, _ptr(dw), _ptr(db), _ptr(ws), _stream())
        return (dx.view(ctx.in_shape) if dx is not None else None), dw, db, None, None, None, None


def row_logit(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, mask: Optional[Tensor] = None, p: float = 0.0, training: bool = False,
              drop: Optional[DropoutState] = None) -> Tensor:
    """[..., H] -> [..., 1] fp32.  `mask` ([...] of 0 / 1, optional) adds (1 - mask) * -10000; dropout with probability p in training mode takes
    its site from `drop` like `dropout`."""
    if training and p > 0.0:
        if drop is None:
            raise RuntimeError("dropout requested without a DropoutState")
        return RowLogitFn.apply(x, weight, bias, mask, p, drop.tensor, drop.next_site())
    return RowLogitFn.apply(x, weight, bias, mask, 0.0, None, 0)


# ------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------
def _eptr(t: Optional[Tensor], offset_elems: int = 0):
    return None if t is None else t.data_ptr() + t.element_size() * offset_elems


def _attn_problem(q, q_off, ldq, k, k_off, ldk, v, v_off, ldv, mask, Tq, Tk, p, site, ctx=None, lse=None, ctx_in=None, dctx=None,
                  lse_in=None, delta=None, dq=None, dq_off=0, lddq=0, dk=None, dk_off=0, lddk=0, dv=None, dv_off=0, lddv=0, keep=None):
    """One `ytvln_attn_problem` record (include/ytvln.h); q / k / v / ctx / gradients are fp32 or bf16 tensors (offsets in elements)."""
    pr = _lib.AttnProblem()
    pr.q, pr.k, pr.v, pr.mask = _eptr(q, q_off), _eptr(k, k_off), _eptr(v, v_off), _ptr(mask)
    pr.ctx, pr.lse = _eptr(ctx), _ptr(lse)
    pr.ctx_in, pr.dctx, pr.lse_in, pr.delta = _eptr(ctx_in), _eptr(dctx), _ptr(lse_in), _ptr(delta)
    pr.dq, pr.dk, pr.dv = _eptr(dq, dq_off), _eptr(dk, dk_off), _eptr(dv, dv_off)
    o = ctx if ctx is not None else ctx_in
    pr.ldq, pr.ldk, pr.ldv, pr.ldo, pr.lddq, pr.lddk, pr.lddv = ldq, ldk, ldv, o.shape[-1], lddq, lddk, lddv
    pr.Tq, pr.Tk, pr.p_drop, pr.site = Tq, Tk, float(p), int(site)
    pr.keep = keep.data_ptr() if keep is not None else None
    return pr


def attn_bias_strides(bias: Tensor, N: int, heads: int, Tq: int, Tk: int) -> Tuple[int, int, int, int]:
    """(stride_n, stride_h, stride_q, stride_k) in elements of a bias that broadcasts against the scores [N, heads, Tq, Tk]
    (`ytvln_attn_bias`, include/ytvln.h): a 4-D tensor or view of shape [N or 1, heads or 1, Tq, Tk], read as it lies -- a dimension of
    size 1 (or an expanded one) gets stride 0, and the transposed view of an [.., Tk, Tq] tensor simply arrives with its strides swapped."""
    if bias.dim() != 4 or bias.shape[0] not in (1, N) or bias.shape[1] not in (1, heads) or tuple(bias.shape[2:]) != (Tq, Tk):
        raise NotImplementedError(f"attention bias of shape {tuple(bias.shape)}: accepted are [N,1,Tq,Tk], [N,heads,Tq,Tk] and [1,1,Tq,Tk] "
                                  f"(N {N}, heads {heads}, Tq {Tq}, Tk {Tk}) or views of those shapes")
    sn, sh, sq, sk = (0 if bias.shape[i] == 1 else int(bias.stride(i)) for i in range(4))
    if sq < 0 or sk < 0:
        raise NotImplementedError("attention bias: negative strides over queries / keys are not supported")
    return sn, sh, sq, sk


def _attn_bias(bias: Optional[Tensor], N: int, heads: int, Tq: int, Tk: int):
    """-> (the tensor the record points into -- keep it alive --, `ytvln_attn_bias` record), or (None, None).  Only an unsupported dtype is
    converted; a non-contiguous view is passed as it lies.  The bias is a constant of the attention: one that requires grad is refused."""
    if bias is None:
        return None, None
    if bias.requires_grad:
        raise RuntimeError("attention bias with requires_grad=True: no gradient with respect to the bias is computed (detach it)")
    if not bias.is_cuda:
        raise RuntimeError("attention bias must live on the GPU (no CPU fallback)")
    if bias.dtype != torch.float32:
        bias = bias.float()
    rec = _lib.AttnBias()
    rec.ptr = bias.data_ptr()
    rec.stride_n, rec.stride_h, rec.stride_q, rec.stride_k = attn_bias_strides(bias, N, heads, Tq, Tk)
    return bias, rec


def _attn_keep(N, heads, Tq, Tk, p, device):
    """bf16-resident attention with dropout: the buffer the forward kernel writes its keep decisions to and the backward kernels read them from
    (`ytvln_attn_problem.keep`); None without dropout."""
    if not p > 0:
        return None
    return torch.empty(int(_lib.load().ytvln_attn_keep_bytes(N, heads, Tq, Tk)), dtype=torch.uint8, device=device)


def _attn_launch(backward: bool, bf16: bool, pa, pb, N, heads, d, scale, rng, ba=None, bb=None):
    """One launch over one problem (pb = None) or the two directions of BertBiAttention; ba / bb: `ytvln_attn_bias` records of the problems
    (launches without one take the entry points they always took)."""
    rp = _ptr(rng) if rng is not None else None
    if ba is not None or bb is not None:
        name = "ytvln_attn_%s_bias_%s" % ("bwd" if backward else "fwd", "bf16" if bf16 else "f32")
        call(name, ctypes.addressof(pa), ctypes.addressof(ba) if ba is not None else None, ctypes.addressof(pb) if pb is not None else None,
             ctypes.addressof(bb) if bb is not None else None, N, heads, d, float(scale), rp, _stream())
    elif bf16:
        call("ytvln_attn_bwd_bf16" if backward else "ytvln_attn_fwd_bf16", ctypes.addressof(pa), ctypes.addressof(pb) if pb is not None else None,
             N, heads, d, float(scale), rp, _stream())
    elif backward:
        ws, n_ws = _attn_bwd_workspace(N, heads, d, pa.Tq, pa.Tk, pb.Tq, pb.Tk, torch.device("cuda", torch.cuda.current_device()))
        call("ytvln_attn_bwd_pair_ws", ctypes.addressof(pa), ctypes.addressof(pb), N, heads, d, float(scale), rp, _ptr(ws), n_ws, _stream())
    else:
        call("ytvln_attn_fwd_pair", ctypes.addressof(pa), ctypes.addressof(pb), N, heads, d, float(scale), rp, _stream())


def _attn_bwd_workspace(N, heads, d, Tq_a, Tk_a, Tq_b, Tk_b, device):
    """-> (tensor or None, floats) of the dS workspace of one fp32 backward launch (`ytvln_attn_bwd_workspace_elems`, include/ytvln.h); 0 floats when
    the launch would not take the stored-dS form.  Allocated per call on the current stream: the caching allocator hands the block to the next
    site once this launch's kernels, which are queued on that stream, are through with it -- safe under graph capture and with the text side on
    its own stream."""
    n = int(_lib.load().ytvln_attn_bwd_workspace_elems(N, heads, d, Tq_a, Tk_a, Tq_b, Tk_b))
    if n == 0:
        return None, 0
    return torch.empty(n, dtype=torch.float32, device=device), n


def _attn_fwd(q, q_off, ldq, k, k_off, ldk, v, v_off, ldv, mask, out, N, heads, Tq, Tk, d, scale, p, rng, site, bias=None):
    lse = torch.empty((N, heads, Tq), dtype=torch.float32, device=out.device)
    bias, brec = _attn_bias(bias, N, heads, Tq, Tk)
    if q.dtype == torch.bfloat16 or brec is not None:
        bf16 = q.dtype == torch.bfloat16
        keep = _attn_keep(N, heads, Tq, Tk, p, out.device) if bf16 else None
        _attn_launch(False, bf16, _attn_problem(q, q_off, ldq, k, k_off, ldk, v, v_off, ldv, mask, Tq, Tk, p, site, ctx=out, lse=lse, keep=keep),
                     None, N, heads, d, scale, rng, ba=brec)
        lse._ytvln_keep = keep          # direct callers hand `lse` to _attn_bwd, which finds the forward's keep decisions here; the autograd
        return lse                      # functions save the buffer explicitly (a saved tensor is unpacked into a new Python object)
    call("ytvln_attn_fwd_f32", _ptr(q, q_off), ldq, _ptr(k, k_off), ldk, _ptr(v, v_off), ldv, _ptr(mask), _ptr(out), out.shape[-1],
         _ptr(lse), N, heads, Tq, Tk, d, float(scale), float(p), _ptr(rng) if rng is not None else None, int(site), _stream())
    return lse


def _attn_bwd(q, q_off, ldq, k, k_off, ldk, v, v_off, ldv, mask, out, dout, lse, dq, dq_off, lddq, dk, dk_off, lddk, dv, dv_off,
              lddv, N, heads, Tq, Tk, d, scale, p, rng, site, keep=None, bias=None):
    delta = torch.empty_like(lse)
    bias, brec = _attn_bias(bias, N, heads, Tq, Tk)
    if q.dtype == torch.bfloat16 or brec is not None:
        bf16 = q.dtype == torch.bfloat16
        if keep is None:
            keep = getattr(lse, "_ytvln_keep", None)
        if bf16 and p > 0 and keep is None:
            raise RuntimeError("bf16 attention backward with dropout needs the keep decisions its forward wrote (pass keep= or the lse tensor _attn_fwd returned)")
        _attn_launch(True, bf16, _attn_problem(q, q_off, ldq, k, k_off, ldk, v, v_off, ldv, mask, Tq, Tk, p, site, ctx_in=out, dctx=dout,
                                               lse_in=lse, delta=delta, dq=dq, dq_off=dq_off, lddq=lddq, dk=dk, dk_off=dk_off, lddk=lddk,
                                               dv=dv, dv_off=dv_off, lddv=lddv, keep=keep), None, N, heads, d, scale, rng, ba=brec)
        return delta
    ws, n_ws = _attn_bwd_workspace(N, heads, d, Tq, Tk, 0, 0, q.device)
    call("ytvln_attn_bwd_ws_f32", _ptr(q, q_off), ldq, _ptr(k, k_off), ldk, _ptr(v, v_off), ldv, _ptr(mask), _ptr(out), _ptr(dout),
         out.shape[-1], _ptr(lse), _ptr(delta), _ptr(dq, dq_off), lddq, _ptr(dk, dk_off), lddk, _ptr(dv, dv_off), lddv, N, heads, Tq,
         Tk, d, float(scale), float(p), _ptr(rng) if rng is not None else None, int(site), _ptr(ws), n_ws, _stream())
    return delta


def _trainable_bias(bias: Optional[Tensor], needs_grad: bool):
    """-> (the tensor the launches read, (shape, dtype) of the gradient to return or None).  A bias that autograd wants a gradient for reaches the
    launches as a detached fp32 view (`_attn_bias` refuses one that requires grad: a raw launch computes no bias gradient); every other bias
    passes through untouched."""
    if bias is None or not needs_grad:
        return bias, None
    b = bias.detach()
    return (b if b.dtype == torch.float32 else b.float()), (tuple(bias.shape), bias.dtype)


def _attn_dbias(pr, bias: Optional[Tensor], like, bf16: bool, N, heads, Tq, Tk, d, scale, rng, device) -> Tensor:
    """Gradient of a trainable per-score bias (`ytvln_attn_dbias_*`, include/ytvln.h), enqueued behind the backward launch of the same problem:
    `pr` is that launch's problem record (its delta buffer is read), `bias` the detached forward values, `like` = (shape, dtype) of the bias
    argument.  The result is a fresh contiguous buffer of that shape: a dimension of size 1 is summed over inside the library; an expanded
    one (stride 0, size > 1) gets its full gradient and autograd's expand-backward sums it; a transposed view gets the gradient of the view."""
    shape, dtype = like
    g = torch.empty(shape, dtype=torch.float32, device=device)
    orec = _lib.AttnBias()
    orec.ptr = g.data_ptr()
    orec.stride_n, orec.stride_h, orec.stride_q, orec.stride_k = attn_bias_strides(g, N, heads, Tq, Tk)
    brec = None
    if bias is not None:
        brec = _lib.AttnBias()
        brec.ptr = bias.data_ptr()
        brec.stride_n, brec.stride_h, brec.stride_q, brec.stride_k = attn_bias_strides(bias, N, heads, Tq, Tk)
    need = int(_lib.load().ytvln_attn_dbias_workspace_elems(ctypes.addressof(orec), N, heads, Tq, Tk))
    ws = torch.empty(need, dtype=torch.float32, device=device) if need > 0 else None
    call("ytvln_attn_dbias_bf16" if bf16 else "ytvln_attn_dbias_f32", ctypes.addressof(pr), ctypes.addressof(brec) if brec is not None else None,
         ctypes.addressof(orec), _ptr(ws), need, N, heads, d, float(scale), _ptr(rng) if rng is not None else None, _stream())
    return g if dtype == torch.float32 else g.to(dtype)


def attn_probs(q, q_off, ldq, k, k_off, ldk, mask, lse, N, heads, Tq, Tk, d, scale, bias=None) -> Tensor:
    probs = torch.empty((N, heads, Tq, Tk), dtype=torch.float32, device=lse.device)
    if q.dtype == torch.bfloat16 or k.dtype == torch.bfloat16:
        # bf16-resident path (output_all_attention_masks is a rare diagnostic there): the probability kernel reads fp32 rows, so the
        # bf16 projections are widened first -- offsets and leading dimensions are in elements and carry over unchanged
        q, k = q.float(), k.float()
    elif q.dtype != torch.float32 or k.dtype != torch.float32:
        raise RuntimeError(f"attn_probs: q / k must be float32 or bfloat16, got {q.dtype} / {k.dtype}")
    bias, brec = _attn_bias(bias, N, heads, Tq, Tk)
    if brec is not None:
        call("ytvln_attn_probs_bias_f32", _ptr(q, q_off), ldq, _ptr(k, k_off), ldk, _ptr(mask), ctypes.addressof(brec), _ptr(lse), _ptr(probs),
             N, heads, Tq, Tk, d, float(scale), _stream())
        return probs
    call("ytvln_attn_probs_f32", _ptr(q, q_off), ldq, _ptr(k, k_off), ldk, _ptr(mask), _ptr(lse), _ptr(probs), N, heads, Tq, Tk, d,
         float(scale), _stream())
    return probs


class SelfAttentionFn(torch.autograd.Function):
    """ctx = MHA(qkv) for a packed [N*T, 3H] projection (query | key | value column blocks); vilbert.py:284-311.
    Optional ninth argument: a per-score additive bias (see `attn_bias_strides`); `mask` may then be None."""

    @staticmethod
    def forward(ctx, qkv, mask, N, T, heads, p, rng, site, *opt):
        bias, ctx.bias_like = _trainable_bias(opt[0] if opt else None, bool(opt) and ctx.needs_input_grad[8])
        ctx.n_in = 8 + len(opt)
        ctx.set_materialize_grads(False)
        _check(qkv, "qkv", qkv.dtype if qkv.dtype == torch.bfloat16 else torch.float32)
        assert qkv.is_contiguous() and qkv.dim() == 2 and qkv.shape[0] == N * T
        H = qkv.shape[1] // 3
        d = H // heads
        if qkv.dtype == torch.bfloat16 and d not in (64, 128):
            raise NotImplementedError(f"bf16-resident attention is built for head dimensions 64 and 128 (got {d}); use the fp32 path")
        scale = 1.0 / math.sqrt(d)
        out = torch.empty((N * T, H), dtype=qkv.dtype, device=qkv.device)
        lse = _attn_fwd(qkv, 0, 3 * H, qkv, H, 3 * H, qkv, 2 * H, 3 * H, mask, out, N, heads, T, T, d, scale, p, rng, site, bias=bias)
        keep = getattr(lse, "_ytvln_keep", None)
        ctx.meta = (N, T, heads, H, d, scale, p, site)
        ctx.save_for_backward(qkv, mask, out, lse, rng, keep, bias)          # (the bias by reference: no copy)
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    def backward(ctx, dout, _dlse):
        if dout is None:
            return (None,) * ctx.n_in
        qkv, mask, out, lse, rng, keep, bias = ctx.saved_tensors
        N, T, heads, H, d, scale, p, site = ctx.meta
        dout = dout if dout.is_contiguous() else dout.contiguous()
        if dout.dtype != qkv.dtype:
            dout = dout.to(qkv.dtype)
        dqkv = torch.empty_like(qkv)
        delta = _attn_bwd(qkv, 0, 3 * H, qkv, H, 3 * H, qkv, 2 * H, 3 * H, mask, out, dout, lse, dqkv, 0, 3 * H, dqkv, H, 3 * H, dqkv, 2 * H,
                          3 * H, N, heads, T, T, d, scale, p, rng, site, keep=keep, bias=bias)
        if ctx.bias_like is None:
            return (dqkv,) + (None,) * (ctx.n_in - 1)
        # trainable bias: dBias = dS, recomputed by a launch of its own behind the backward (unfused by design, include/ytvln.h)
        pr = _attn_problem(qkv, 0, 3 * H, qkv, H, 3 * H, qkv, 2 * H, 3 * H, mask, T, T, p, site, ctx_in=out, dctx=dout, lse_in=lse, delta=delta,
                           keep=keep)
        gb = _attn_dbias(pr, bias, ctx.bias_like, qkv.dtype == torch.bfloat16, N, heads, T, T, d, scale, rng, qkv.device)
        return (dqkv,) + (None,) * 7 + (gb,)


class CoAttentionFn(torch.autograd.Function):
    """BertBiAttention (vilbert.py:552-618).  Projections are packed PER DIRECTION so that a direction whose context is
    never used downstream (e.g. the vision side of the last co-layer under --masked_language only) propagates `None`
    gradients exactly like the reference's autograd graph -- AdamW must not touch those tensors:
        q1  [N*R, Hb]  = query1(image)        kv1 [N*R, 2Hb] = key1|value1(image)
        q2  [N*T, Hb]  = query2(text)         kv2 [N*T, 2Hb] = key2|value2(text)
        ctx1 [N*T, Hb] = attend(q2; kv1, image mask)     ctx2 [N*R, Hb] = attend(q1; kv2, text mask)"""

    @staticmethod
    def forward(ctx, q1, kv1, q2, kv2, mask1, mask2, N, R, T, heads, p1, p2, rng, site1, site2, *opt):
        """opt: (bias1, bias2) -- per-score biases of the two directions, [.., T, R] for ctx1 and [.., R, T] for ctx2 (either may be None)."""
        bias1, bias2 = (tuple(opt) + (None, None))[:2]
        ctx.n_in = 15 + len(opt)
        bias1, ctx.bias1_like = _trainable_bias(bias1, len(opt) > 0 and ctx.needs_input_grad[15])
        bias2, ctx.bias2_like = _trainable_bias(bias2, len(opt) > 1 and ctx.needs_input_grad[16])
        bias1, b1 = _attn_bias(bias1, N, heads, T, R)
        bias2, b2 = _attn_bias(bias2, N, heads, R, T)
        bf16 = q1.dtype == torch.bfloat16
        for t, nme in ((q1, "q1"), (kv1, "kv1"), (q2, "q2"), (kv2, "kv2")):
            _check(t, nme, torch.bfloat16 if bf16 else torch.float32)
            assert t.is_contiguous() and t.dim() == 2
        Hb = q1.shape[1]
        d = Hb // heads
        if bf16 and d not in (64, 128):
            raise NotImplementedError(f"bf16-resident attention is built for head dimensions 64 and 128 (got {d}); use the fp32 path")
        scale = 1.0 / math.sqrt(d)
        ctx1 = torch.empty((N * T, Hb), dtype=q1.dtype, device=q1.device)
        ctx2 = torch.empty((N * R, Hb), dtype=q1.dtype, device=q1.device)
        lse1 = torch.empty((N, heads, T), dtype=torch.float32, device=q1.device)
        lse2 = torch.empty((N, heads, R), dtype=torch.float32, device=q1.device)
        # both directions in one launch (text queries over regions | region queries over text)
        pk = max(p1, p2)          # one launch: dropout in either direction makes the kernels record decisions for both
        keep1 = _attn_keep(N, heads, T, R, pk, q1.device) if bf16 else None
        keep2 = _attn_keep(N, heads, R, T, pk, q1.device) if bf16 else None
        _attn_launch(False, bf16,
                     _attn_problem(q2, 0, Hb, kv1, 0, 2 * Hb, kv1, Hb, 2 * Hb, mask1, T, R, p1, site1, ctx=ctx1, lse=lse1, keep=keep1),
                     _attn_problem(q1, 0, Hb, kv2, 0, 2 * Hb, kv2, Hb, 2 * Hb, mask2, R, T, p2, site2, ctx=ctx2, lse=lse2, keep=keep2),
                     N, heads, d, scale, rng, ba=b1, bb=b2)
        ctx.meta = (N, R, T, heads, Hb, d, scale, p1, p2, site1, site2)
        ctx.save_for_backward(q1, kv1, q2, kv2, mask1, mask2, ctx1, ctx2, lse1, lse2, rng, keep1, keep2, bias1, bias2)
        ctx.mark_non_differentiable(lse1, lse2)
        ctx.set_materialize_grads(False)
        return ctx1, ctx2, lse1, lse2

    @staticmethod
    def backward(ctx, d1, d2, _a, _b):
        q1, kv1, q2, kv2, mask1, mask2, ctx1, ctx2, lse1, lse2, rng, keep1, keep2, bias1, bias2 = ctx.saved_tensors
        N, R, T, heads, Hb, d, scale, p1, p2, site1, site2 = ctx.meta
        nn_ = (None,) * (ctx.n_in - 4)
        gq1 = gkv1 = gq2 = gkv2 = None
        bf16 = q1.dtype == torch.bfloat16
        want1, want2 = ctx.bias1_like is not None, ctx.bias2_like is not None          # trainable biases: each live direction's gets its own gradient

        def tail(gb1, gb2):
            return nn_ if not (want1 or want2) else (None,) * 11 + (gb1, gb2)[:ctx.n_in - 15]
        if d1 is not None and d2 is not None:       # the usual case: both directions in one launch per kernel
            d1 = d1 if d1.is_contiguous() else d1.contiguous()
            d2 = d2 if d2.is_contiguous() else d2.contiguous()
            gq2, gkv1, gq1, gkv2 = torch.empty_like(q2), torch.empty_like(kv1), torch.empty_like(q1), torch.empty_like(kv2)
            delta1, delta2 = torch.empty_like(lse1), torch.empty_like(lse2)
            pa = _attn_problem(q2, 0, Hb, kv1, 0, 2 * Hb, kv1, Hb, 2 * Hb, mask1, T, R, p1, site1, ctx_in=ctx1, dctx=d1, lse_in=lse1,
                               delta=delta1, dq=gq2, lddq=Hb, dk=gkv1, lddk=2 * Hb, dv=gkv1, dv_off=Hb, lddv=2 * Hb, keep=keep1)
            pb = _attn_problem(q1, 0, Hb, kv2, 0, 2 * Hb, kv2, Hb, 2 * Hb, mask2, R, T, p2, site2, ctx_in=ctx2, dctx=d2, lse_in=lse2,
                               delta=delta2, dq=gq1, lddq=Hb, dk=gkv2, lddk=2 * Hb, dv=gkv2, dv_off=Hb, lddv=2 * Hb, keep=keep2)
            _attn_launch(True, bf16, pa, pb, N, heads, d, scale, rng, ba=_attn_bias(bias1, N, heads, T, R)[1],
                         bb=_attn_bias(bias2, N, heads, R, T)[1])
            gb1 = _attn_dbias(pa, bias1, ctx.bias1_like, bf16, N, heads, T, R, d, scale, rng, q1.device) if want1 else None
            gb2 = _attn_dbias(pb, bias2, ctx.bias2_like, bf16, N, heads, R, T, d, scale, rng, q1.device) if want2 else None
            return (gq1, gkv1, gq2, gkv2) + tail(gb1, gb2)
        gb1 = gb2 = None          # (a direction whose context gradient is None returns None for its bias)
        if d1 is not None:      # text queries over image keys/values -> dq2, dk1|dv1
            d1 = d1 if d1.is_contiguous() else d1.contiguous()
            gq2, gkv1 = torch.empty_like(q2), torch.empty_like(kv1)
            delta1 = _attn_bwd(q2, 0, Hb, kv1, 0, 2 * Hb, kv1, Hb, 2 * Hb, mask1, ctx1, d1, lse1, gq2, 0, Hb, gkv1, 0, 2 * Hb, gkv1, Hb,
                               2 * Hb, N, heads, T, R, d, scale, p1, rng, site1, keep=keep1, bias=bias1)
            if want1:
                pa = _attn_problem(q2, 0, Hb, kv1, 0, 2 * Hb, kv1, Hb, 2 * Hb, mask1, T, R, p1, site1, ctx_in=ctx1, dctx=d1, lse_in=lse1,
                                   delta=delta1, keep=keep1)
                gb1 = _attn_dbias(pa, bias1, ctx.bias1_like, bf16, N, heads, T, R, d, scale, rng, q1.device)
        if d2 is not None:      # image queries over text keys/values -> dq1, dk2|dv2
            d2 = d2 if d2.is_contiguous() else d2.contiguous()
            gq1, gkv2 = torch.empty_like(q1), torch.empty_like(kv2)
            delta2 = _attn_bwd(q1, 0, Hb, kv2, 0, 2 * Hb, kv2, Hb, 2 * Hb, mask2, ctx2, d2, lse2, gq1, 0, Hb, gkv2, 0, 2 * Hb, gkv2, Hb,
                               2 * Hb, N, heads, R, T, d, scale, p2, rng, site2, keep=keep2, bias=bias2)
            if want2:
                pb = _attn_problem(q1, 0, Hb, kv2, 0, 2 * Hb, kv2, Hb, 2 * Hb, mask2, R, T, p2, site2, ctx_in=ctx2, dctx=d2, lse_in=lse2,
                                   delta=delta2, keep=keep2)
                gb2 = _attn_dbias(pb, bias2, ctx.bias2_like, bf16, N, heads, R, T, d, scale, rng, q1.device)
        return (gq1, gkv1, gq2, gkv2) + tail(gb1, gb2)


# ------------------------------------------------------------------------------------------------------------------
# losses
# ------------------------------------------------------------------------------------------------------------------
class CrossEntropyFn(torch.autograd.Function):
    """F.cross_entropy(logits, target, ignore_index) with mean reduction (utils_init.py:133-135, :141)."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index):
        ctx.set_materialize_grads(False)
        bf = logits.dtype == _BF16             # bf16-resident path: bf16 logits in, bf16 gradient out (same kernels, 2-byte loads/stores)
        lg, M, V, ld = _format_of(logits).rows(logits, "logits")
        tg = _i64(target, "target").reshape(-1)
        assert tg.numel() == M, (tg.shape, M)
        dev = lg.device
        row_lse = torch.empty(M, dtype=torch.float32, device=dev)
        row_loss = torch.empty(M, dtype=torch.float32, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        call("ytvln_ce_fwd_bf16" if bf else "ytvln_ce_fwd_f32", lg.data_ptr(), ld, _ptr(tg), int(ignore_index), _ptr(row_lse), _ptr(row_loss),
             _ptr(out), M, V, _stream())
        ctx.meta = (M, V, ld, int(ignore_index), logits.shape)
        ctx.bf16_grad = bf
        ctx.save_for_backward(lg, tg, row_lse, out)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None
        lg, tg, row_lse, out = ctx.saved_tensors
        M, V, ld, ign, shape = ctx.meta
        g = g.reshape(1).contiguous().float()
        if ctx.bf16_grad:          # rounded once, zero padding written by the kernel: feeds ytvln_gemm_bf16 as it stands
            dl, ldd = _alloc_rows_bf16(M, V, lg.device)
            call("ytvln_ce_bwd_bf16", lg.data_ptr(), ld, _ptr(tg), ign, _ptr(row_lse), _ptr(out), _ptr(g), dl.data_ptr(), ldd, M, V, _stream())
            return _view_rows_as(dl, ldd, shape), None, None
        dl, ldd = _F32.alloc_rows(M, V, lg.device, zero_pad=True)
        call("ytvln_ce_bwd_f32", _ptr(lg), ld, _ptr(tg), ign, _ptr(row_lse), _ptr(out), _ptr(g), _ptr(dl), ldd, M, V, _stream())
        return _view_rows_as(dl, ldd, shape), None, None


def _label_smoothing(value) -> float:
    """`label_smoothing` as a float in [0, 1), or ValueError (before anything is launched)."""
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not 0.0 <= float(value) < 1.0:       # a NaN fails both comparisons
        raise ValueError(f"label_smoothing must be a real number in [0, 1), got {value!r}")
    return float(value)


class CrossEntropyStatsFn(torch.autograd.Function):
    """CrossEntropyFn with label smoothing and, from the same pass over the logits, the row arg-max, the hits and the row count."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index, eps):
        ctx.set_materialize_grads(False)
        bf = logits.dtype == _BF16
        lg, M, V, ld = _format_of(logits).rows(logits, "logits")
        tg = _i64(target, "target").reshape(-1)
        assert tg.numel() == M, (tg.shape, M)
        dev = lg.device
        row_lse = torch.empty(M, dtype=torch.float32, device=dev)
        row_nv = torch.empty(M, dtype=torch.float32, device=dev)
        row_loss = torch.empty(M, dtype=torch.float32, device=dev)
        row_top = torch.empty(M, dtype=torch.int64, device=dev)
        out = torch.empty(4, dtype=torch.float32, device=dev)
        call("ytvln_ce_stats_fwd_bf16" if bf else "ytvln_ce_stats_fwd_f32", lg.data_ptr(), ld, _ptr(tg), int(ignore_index), eps, _ptr(row_lse),
             _ptr(row_nv), _ptr(row_loss), row_top.data_ptr(), _ptr(out), M, V, _stream())
        ctx.meta = (M, V, ld, int(ignore_index), eps, logits.shape)
        ctx.bf16_grad = bf
        ctx.save_for_backward(lg, tg, row_lse, row_nv, out)
        loss, hits, count = out[0], out[2], out[3]
        ctx.mark_non_differentiable(hits, count, row_top)
        return loss, hits, count, row_top

    @staticmethod
    def backward(ctx, g, _ghits=None, _gcount=None, _gtop=None):
        if g is None:
            return None, None, None, None
        lg, tg, row_lse, row_nv, out = ctx.saved_tensors
        M, V, ld, ign, eps, shape = ctx.meta
        g = g.reshape(1).contiguous().float()
        sfx = "bf16" if ctx.bf16_grad else "f32"
        if ctx.bf16_grad:
            dl, ldd = _alloc_rows_bf16(M, V, lg.device)
        else:
            dl, ldd = _F32.alloc_rows(M, V, lg.device, zero_pad=True)
        if eps == 0.0:          # no smoothing: the plain backward as it stands
            call("ytvln_ce_bwd_" + sfx, lg.data_ptr(), ld, _ptr(tg), ign, _ptr(row_lse), _ptr(out), _ptr(g), dl.data_ptr(), ldd, M, V, _stream())
        else:
            call("ytvln_ce_smooth_bwd_" + sfx, lg.data_ptr(), ld, _ptr(tg), ign, eps, _ptr(row_lse), _ptr(row_nv), _ptr(out), _ptr(g),
                 dl.data_ptr(), ldd, M, V, _stream())
        return _view_rows_as(dl, ldd, shape), None, None, None


def cross_entropy(logits: Tensor, target: Tensor, ignore_index: int = -100, label_smoothing: float = 0.0) -> Tensor:
    """F.cross_entropy(logits, target, ignore_index=ignore_index, label_smoothing=label_smoothing), mean reduction.  With smoothing, -inf
    logits (padded options) take no share of the smoothing mass: see cross_entropy_stats."""
    eps = _label_smoothing(label_smoothing)
    if eps == 0.0:
        return CrossEntropyFn.apply(logits, target, ignore_index)
    return CrossEntropyStatsFn.apply(logits, target, ignore_index, eps)[0]


def cross_entropy_stats(logits: Tensor, target: Tensor, ignore_index: int = -100,
                        label_smoothing: float = 0.0) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(loss, hits, count, row_top) from one pass over the logits, without a host sync:
    loss = the label-smoothed cross entropy, mean over the rows whose target is not `ignore_index` (0-d, differentiable in `logits`; NaN when
    there is no such row).  Row loss = (1 - eps)(lse - x[t]) + eps (lse - mean of the row's logits that are not -inf): F.cross_entropy's value
    when no logit is -inf; with -inf logits the smoothing mass goes to the other classes only (torch gives +inf there), and the gradient of a
    -inf column is 0.  With label_smoothing = 0 the loss and its gradient are cross_entropy's, bit for bit.
    row_top = int64 [M], the arg-max of each row: lowest index among equals, a NaN counts as the maximum (torch.argmax); -1 for an ignored row.
    hits = number of non-ignored rows with row_top == target, count = number of non-ignored rows (0-d fp32, exact up to 2^24 rows)."""
    return CrossEntropyStatsFn.apply(logits, target, ignore_index, _label_smoothing(label_smoothing))


class KLMaskedFn(torch.autograd.Function):
    """sum(mask * kl_div(log_softmax(pred), target)) / max(1, sum(mask))  (utils_init.py:117-128), no host sync."""

    @staticmethod
    def forward(ctx, pred, target, mask):
        ctx.set_materialize_grads(False)
        bf = pred.dtype == _BF16
        pr, M, Cc, ld = _format_of(pred).rows(pred, "pred")
        tg, M2, C2, ldt = _F32.rows(target, "target")
        assert (M, Cc) == (M2, C2), (pred.shape, target.shape)
        mk = _i64(mask, "mask").reshape(-1)
        dev = pr.device
        row_lse = torch.empty(M, dtype=torch.float32, device=dev)
        row_loss = torch.empty(M, dtype=torch.float32, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        call("ytvln_kl_fwd_bf16" if bf else "ytvln_kl_fwd_f32", pr.data_ptr(), ld, _ptr(tg), ldt, _ptr(mk), _ptr(row_lse), _ptr(row_loss),
             _ptr(out), M, Cc, _stream())
        ctx.meta = (M, Cc, ld, ldt, pred.shape)
        ctx.bf16_grad = bf
        ctx.save_for_backward(pr, tg, mk, row_lse, out)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None
        pr, tg, mk, row_lse, out = ctx.saved_tensors
        M, Cc, ld, ldt, shape = ctx.meta
        g = g.reshape(1).contiguous().float()
        if ctx.bf16_grad:
            dp, ldd = _alloc_rows_bf16(M, Cc, pr.device)
            call("ytvln_kl_bwd_bf16", pr.data_ptr(), ld, _ptr(tg), ldt, _ptr(mk), _ptr(row_lse), _ptr(out), _ptr(g), dp.data_ptr(), ldd, M, Cc, _stream())
            return _view_rows_as(dp, ldd, shape), None, None
        dp, ldd = _F32.alloc_rows(M, Cc, pr.device, zero_pad=True)
        call("ytvln_kl_bwd_f32", _ptr(pr), ld, _ptr(tg), ldt, _ptr(mk), _ptr(row_lse), _ptr(out), _ptr(g), _ptr(dp), ldd, M, Cc, _stream())
        return _view_rows_as(dp, ldd, shape), None, None


def kl_masked(pred: Tensor, target: Tensor, mask: Tensor) -> Tensor:
    return KLMaskedFn.apply(pred, target, mask)


class KLMaskedStatsFn(torch.autograd.Function):
    """KLMaskedFn plus, from the same pass, the arg-max of every prediction row and how many of them agree with the target row's."""

    @staticmethod
    def forward(ctx, pred, target, mask):
        ctx.set_materialize_grads(False)
        bf = pred.dtype == _BF16
        pr, M, Cc, ld = _format_of(pred).rows(pred, "pred")
        tg, M2, C2, ldt = _F32.rows(target, "target")
        assert (M, Cc) == (M2, C2), (pred.shape, target.shape)
        mk = _i64(mask, "mask").reshape(-1)
        dev = pr.device
        row_lse = torch.empty(M, dtype=torch.float32, device=dev)
        row_loss = torch.empty(M, dtype=torch.float32, device=dev)
        row_hit = torch.empty(M, dtype=torch.float32, device=dev)
        row_top = torch.empty(M, dtype=torch.int64, device=dev)
        out = torch.empty(4, dtype=torch.float32, device=dev)
        call("ytvln_kl_stats_fwd_bf16" if bf else "ytvln_kl_stats_fwd_f32", pr.data_ptr(), ld, _ptr(tg), ldt, _ptr(mk), _ptr(row_lse),
             _ptr(row_loss), row_top.data_ptr(), _ptr(row_hit), _ptr(out), M, Cc, _stream())
        ctx.meta = (M, Cc, ld, ldt, pred.shape)
        ctx.bf16_grad = bf
        ctx.save_for_backward(pr, tg, mk, row_lse, out)
        loss, hits, count = out[0], out[2], out[3]
        ctx.mark_non_differentiable(hits, count, row_top)
        return loss, hits, count, row_top

    @staticmethod
    def backward(ctx, g, _ghits=None, _gcount=None, _gtop=None):          # ytvln_kl_bwd_* reads out[1] only: the plain backward serves
        return KLMaskedFn.backward(ctx, g)


def kl_masked_stats(pred: Tensor, target: Tensor, mask: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(loss, hits, count, row_top): kl_masked's loss (same bits, same gradient) and, from the same pass, row_top = int64 [M] arg-max of each
    prediction row (lowest index among equals, a NaN counts as the maximum; -1 where mask == 0), hits = number of rows with mask != 0 whose
    arg-max equals the target row's, count = number of rows with mask != 0 (0-d fp32, not clamped).  No host sync."""
    return KLMaskedStatsFn.apply(pred, target, mask)


class BCEWithLogitsFn(torch.autograd.Function):
    """F.binary_cross_entropy_with_logits(x, t, pos_weight=w), mean reduction (utils_init.py:143, :160-161)."""

    @staticmethod
    def forward(ctx, x, t, pos_weight):
        ctx.set_materialize_grads(False)
        _check(x, "x")
        xc = x.contiguous()
        tc = t.to(torch.float32).contiguous()
        pw = pos_weight.to(torch.float32).reshape(1).contiguous() if pos_weight is not None else None
        out = torch.empty(1, dtype=torch.float32, device=x.device)
        call("ytvln_bce_fwd_f32", _ptr(xc), _ptr(tc), _ptr(pw), _ptr(out), xc.numel(), _stream())
        ctx.save_for_backward(xc, tc, pw)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None
        xc, tc, pw = ctx.saved_tensors
        g = g.reshape(1).contiguous().float()
        dx = torch.empty_like(xc)
        call("ytvln_bce_bwd_f32", _ptr(xc), _ptr(tc), _ptr(pw), _ptr(g), _ptr(dx), xc.numel(), _stream())
        return dx, None, None


def bce_with_logits(x: Tensor, t: Tensor, pos_weight: Optional[Tensor] = None) -> Tensor:
    return BCEWithLogitsFn.apply(x, t, pos_weight)


class BCERowsFn(torch.autograd.Function):
    """scale * mean(bce_with_logits(x, t, pos_weight)) over a [M, C] matrix of any size, with the row arg-max and the sum of the targets at it
    (the score of a soft-target classification task) from the same pass.  fp32 logits only: both producers of such logits write fp32."""

    @staticmethod
    def forward(ctx, x, t, pos_weight, scale):
        ctx.set_materialize_grads(False)
        x2, M, Cc, ldx = _F32.rows(x, "x")
        if not t.is_cuda:
            raise RuntimeError(f"ytvln.ops: `t` must live on the GPU (no CPU fallback); got device {t.device}")
        t2, M2, C2, ldt = _F32.rows(t if t.dtype == torch.float32 else t.to(torch.float32), "t")
        if (M, Cc) != (M2, C2):
            raise RuntimeError(f"ytvln.ops.bce_with_logits_rows: logits {tuple(x.shape)} against targets {tuple(t.shape)}")
        pw, pw_stride = None, 0
        if pos_weight is not None:
            if pos_weight.numel() not in (1, Cc):
                raise RuntimeError(f"ytvln.ops.bce_with_logits_rows: pos_weight of {pos_weight.numel()} elements for {Cc} classes")
            pw = pos_weight.to(torch.float32).reshape(-1).contiguous()
            _check(pw, "pos_weight")
            pw_stride = 1 if pw.numel() == Cc and Cc > 1 else 0
        dev = x2.device
        row_loss = torch.empty(M, dtype=torch.float32, device=dev)
        row_hit = torch.empty(M, dtype=torch.float32, device=dev)
        row_top = torch.empty(M, dtype=torch.int64, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        call("ytvln_bce_rows_fwd_f32", _ptr(x2), ldx, _ptr(t2), ldt, _ptr(pw), pw_stride, float(scale), _ptr(row_loss), _ptr(row_hit),
             row_top.data_ptr(), _ptr(out), M, Cc, _stream())
        ctx.meta = (M, Cc, ldx, ldt, pw_stride, float(scale), x.shape)
        ctx.save_for_backward(x2, t2, pw)
        loss, score = out[0], out[1]
        ctx.mark_non_differentiable(score, row_top)
        return loss, score, row_top

    @staticmethod
    def backward(ctx, g, _gscore=None, _gtop=None):
        if g is None:
            return None, None, None, None
        x2, t2, pw = ctx.saved_tensors
        M, Cc, ldx, ldt, pw_stride, scale, shape = ctx.meta
        g = g.reshape(1).contiguous().float()
        dx, lddx = _F32.alloc_rows(M, Cc, x2.device, zero_pad=True)
        call("ytvln_bce_rows_bwd_f32", _ptr(x2), ldx, _ptr(t2), ldt, _ptr(pw), pw_stride, scale, _ptr(g), _ptr(dx), lddx, M, Cc, _stream())
        return _view_rows_as(dx, lddx, shape), None, None, None


def bce_with_logits_rows(x: Tensor, t: Tensor, pos_weight: Optional[Tensor] = None, scale: float = 1.0) -> Tuple[Tensor, Tensor, Tensor]:
    """(loss, score, row_top) of a [..., C] logit matrix of any size against soft targets of the same shape:
    loss = scale * F.binary_cross_entropy_with_logits(x, t, pos_weight=pos_weight) (0-d, differentiable in x), row_top[r] = argmax of row r
    (int64, lowest index among equals), score = sum_r t[r, row_top[r]] (0-d).  `pos_weight`: None, one element, or [C].  A padded LinearFn
    output is read through its leading dimension, without a copy."""
    return BCERowsFn.apply(x, t, pos_weight, scale)


# ------------------------------------------------------------------------------------------------------------------
# optimizer kernel
# ------------------------------------------------------------------------------------------------------------------
def adamw_step(p: Tensor, g: Tensor, m: Tensor, v: Tensor, chunks: Tensor, nchunks: int, hyper: Tensor, grad_scale: float = 1.0,
               p_bf16: Optional[Tensor] = None):
    """`p_bf16`: the bf16 parameter arena of the bf16-resident path (same offsets): refreshed by the same kernel pass."""
    for t, nme in ((p, "p"), (g, "g"), (m, "m"), (v, "v"), (hyper, "hyper")):
        _check(t, nme)
    if p_bf16 is not None:
        call("ytvln_adamw_f32_bf16copy", _ptr(p), _ptr(g), _ptr(m), _ptr(v), p_bf16.data_ptr(), chunks.data_ptr(), int(nchunks), _ptr(hyper),
             float(grad_scale), _stream())
        return
    call("ytvln_adamw_f32", _ptr(p), _ptr(g), _ptr(m), _ptr(v), chunks.data_ptr(), int(nchunks), _ptr(hyper), float(grad_scale),
         _stream())


def adamw_step_gbf16(p: Tensor, g_bf16: Tensor, m: Tensor, v: Tensor, chunks: Tensor, nchunks: int, hyper: Tensor, grad_scale: float = 1.0,
                     p_bf16: Optional[Tensor] = None):
    """adamw_step reading bf16 gradients (the sums of the bf16 data-parallel exchange, same offsets as the fp32 arena): bit-identical to
    adamw_step fed `g_bf16.float()`."""
    for t, nme in ((p, "p"), (m, "m"), (v, "v"), (hyper, "hyper")):
        _check(t, nme)
    _check(g_bf16, "g_bf16", torch.bfloat16)
    call("ytvln_adamw_f32_gbf16", _ptr(p), g_bf16.data_ptr(), _ptr(m), _ptr(v), None if p_bf16 is None else p_bf16.data_ptr(), chunks.data_ptr(),
         int(nchunks), _ptr(hyper), float(grad_scale), _stream())


def grad_pack_bf16(g: Tensor, g_bf16: Tensor, chunks: Tensor, nchunks: int):
    """g_bf16[o:o+len] = g[o:o+len].to(bfloat16) for every record (offset, length, ...) of an AdamW chunk table, on the current stream."""
    _check(g, "g")
    _check(g_bf16, "g_bf16", torch.bfloat16)
    call("ytvln_grad_pack_bf16", _ptr(g), g_bf16.data_ptr(), chunks.data_ptr(), int(nchunks), _stream())


def _grad_dtype(g: Tensor) -> int:
    if g.dtype == torch.float32:
        return _lib.DT_F32
    if g.dtype == torch.bfloat16:
        return _lib.DT_BF16
    raise RuntimeError(f"gradients must be float32 or bfloat16, got {g.dtype}")


def grad_sumsq(g: Tensor, chunks: Tensor, nchunks: int, partials: Tensor):
    """partials[i] = sum(g[o:o+len] ** 2) for record i of an AdamW chunk table (`g`: the fp32 gradient arena or the bf16 exchange buffer),
    one float per record, on the current stream.  `partials` is a float32 view with room for `nchunks` values."""
    dt = _grad_dtype(g)
    _check(g, "g", g.dtype)
    _check(partials, "partials")
    if partials.numel() < int(nchunks):
        raise RuntimeError(f"grad_sumsq: {int(nchunks)} records, room for {partials.numel()} partials")
    call("ytvln_grad_sumsq", g.data_ptr(), dt, chunks.data_ptr(), int(nchunks), _ptr(partials), _stream())


def grad_clip_coef(partials: Tensor, n: int, grad_scale: float, max_norm: float, skip_nonfinite: bool, clip: Tensor):
    """clip = [norm, coef, skip, skipped steps] from the first `n` partials (include/ytvln.h: ytvln_grad_clip_coef), on the current stream.
    `max_norm` = inf measures without clipping."""
    _check(partials, "partials")
    _check(clip, "clip")
    if clip.numel() != 4 or partials.numel() < int(n):
        raise RuntimeError("grad_clip_coef: clip is a record of 4 floats and partials must hold n values")
    call("ytvln_grad_clip_coef", _ptr(partials), int(n), float(grad_scale), float(max_norm), int(bool(skip_nonfinite)), _ptr(clip), _stream())


def adamw_step_clip(p: Tensor, g: Tensor, m: Tensor, v: Tensor, chunks: Tensor, nchunks: int, hyper: Tensor, clip: Tensor,
                    grad_scale: float = 1.0, p_bf16: Optional[Tensor] = None):
    """adamw_step / adamw_step_gbf16 (by the dtype of `g`) with the gradient scale grad_scale * clip[1] read from the device record of
    grad_clip_coef; a no-op when clip[2] != 0."""
    for t, nme in ((p, "p"), (m, "m"), (v, "v"), (hyper, "hyper"), (clip, "clip")):
        _check(t, nme)
    dt = _grad_dtype(g)
    _check(g, "g", g.dtype)
    call("ytvln_adamw_clip", _ptr(p), g.data_ptr(), dt, _ptr(m), _ptr(v), None if p_bf16 is None else p_bf16.data_ptr(),
         chunks.data_ptr(), int(nchunks), _ptr(hyper), float(grad_scale), _ptr(clip), _stream())


def _check_i32(t: Tensor, name: str, n: int):
    if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous() or t.numel() < n:
        raise RuntimeError(f"{name} must be a contiguous int32 GPU tensor of at least {n} entries")


def lamb_stage1(p: Tensor, g: Tensor, m: Tensor, v: Tensor, chunks: Tensor, nchunks: int, hyper: Tensor, partials: Tensor,
                grad_scale: float = 1.0, clip: Optional[Tensor] = None):
    """First pass of the LAMB update (include/ytvln.h: ytvln_lamb_stage1) over an AdamW chunk table, on the current stream: the moments, and
    partials[2i], partials[2i+1] = sum p^2, sum r^2 of record i.  `g`: the fp32 gradient arena or the bf16 exchange buffer; `clip`: the
    record of grad_clip_coef or None."""
    for t, nme in ((p, "p"), (m, "m"), (v, "v"), (hyper, "hyper"), (partials, "partials")) + (((clip, "clip"),) if clip is not None else ()):
        _check(t, nme)
    dt = _grad_dtype(g)
    _check(g, "g", g.dtype)
    if partials.numel() < 2 * int(nchunks):
        raise RuntimeError(f"lamb_stage1: {int(nchunks)} records, room for {partials.numel() // 2} pairs of partials")
    call("ytvln_lamb_stage1", _ptr(p), g.data_ptr(), dt, _ptr(m), _ptr(v), chunks.data_ptr(), int(nchunks), _ptr(hyper), float(grad_scale),
         _ptr(clip), _ptr(partials), _stream())


def lamb_trust(partials: Tensor, chunks: Tensor, nchunks: int, tensor_first: Tensor, rec_tensor: Tensor, ntensors: int, trust: Tensor,
               report: Tensor, clip: Optional[Tensor] = None):
    """trust[k] and report[k] = [||p||, ||r||, trust, 0] for every tensor of a chunk table from the partials of lamb_stage1
    (include/ytvln.h: ytvln_lamb_trust), on the current stream.  `tensor_first` (ntensors + 1 entries) and `rec_tensor` (one per record)
    are the int32 tables of ytvln.optimization.lamb_tables; trust and report are indexed by rec_tensor's values."""
    for t, nme in ((partials, "partials"), (trust, "trust"), (report, "report")) + (((clip, "clip"),) if clip is not None else ()):
        _check(t, nme)
    _check_i32(tensor_first, "tensor_first", int(ntensors) + 1)
    _check_i32(rec_tensor, "rec_tensor", int(nchunks))
    if partials.numel() < 2 * int(nchunks) or report.numel() != 4 * trust.numel():
        raise RuntimeError("lamb_trust: partials must hold two values per record and report four per entry of trust")
    call("ytvln_lamb_trust", _ptr(partials), chunks.data_ptr(), tensor_first.data_ptr(), rec_tensor.data_ptr(), int(ntensors), _ptr(trust),
         _ptr(report), _ptr(clip), _stream())


def lamb_stage2(p: Tensor, m: Tensor, v: Tensor, chunks: Tensor, nchunks: int, hyper: Tensor, trust: Tensor, rec_tensor: Tensor,
                clip: Optional[Tensor] = None, p_bf16: Optional[Tensor] = None):
    """Second pass of the LAMB update (include/ytvln.h: ytvln_lamb_stage2): p -= lr * trust[rec_tensor[i]] * r over the chunk table, on the
    current stream; `p_bf16` as in adamw_step."""
    for t, nme in ((p, "p"), (m, "m"), (v, "v"), (hyper, "hyper"), (trust, "trust")) + (((clip, "clip"),) if clip is not None else ()):
        _check(t, nme)
    _check_i32(rec_tensor, "rec_tensor", int(nchunks))
    call("ytvln_lamb_stage2", _ptr(p), _ptr(m), _ptr(v), None if p_bf16 is None else p_bf16.data_ptr(), chunks.data_ptr(), int(nchunks),
         _ptr(hyper), _ptr(trust), rec_tensor.data_ptr(), _ptr(clip), _stream())


def ema_update(p: Tensor, e: Tensor, chunks: Tensor, nchunks: int, hyper: Tensor, clip: Optional[Tensor] = None):
    """e = fma(w, p - e, e) with w = hyper[6] over an AdamW chunk table (include/ytvln.h: ytvln_ema_update), on the current stream: the EMA
    of the weights behind an update launch.  `clip`: the record of grad_clip_coef or None; a skipped step leaves `e` untouched."""
    for t, nme in ((p, "p"), (e, "e"), (hyper, "hyper")) + (((clip, "clip"),) if clip is not None else ()):
        _check(t, nme)
    if e.numel() != p.numel() or hyper.numel() < 8:
        raise RuntimeError("ema_update: the shadow arena must have the size of the parameter arena and hyper eight floats")
    call("ytvln_ema_update", _ptr(p), _ptr(e), chunks.data_ptr(), int(nchunks), _ptr(hyper), _ptr(clip), _stream())


def ema_swap(p: Tensor, e: Tensor, chunks: Tensor, nchunks: int, p_bf16: Optional[Tensor] = None):
    """Exchange p and e over an AdamW chunk table (include/ytvln.h: ytvln_ema_swap), on the current stream; `p_bf16` as in adamw_step: the
    bf16 copy of the new p is written by the same pass."""
    _check(p, "p")
    _check(e, "e")
    if p_bf16 is not None:
        _check(p_bf16, "p_bf16", torch.bfloat16)
    if e.numel() != p.numel() or (p_bf16 is not None and p_bf16.numel() != p.numel()):
        raise RuntimeError("ema_swap: the shadow arena and the bf16 copy must have the size of the parameter arena")
    call("ytvln_ema_swap", _ptr(p), _ptr(e), None if p_bf16 is None else p_bf16.data_ptr(), chunks.data_ptr(), int(nchunks), _stream())


def _check_stats_partials(partials: Tensor, bad: Tensor, nchunks: int, who: str):
    _check(partials, "partials")
    if not bad.is_cuda or bad.dtype != torch.int32 or not bad.is_contiguous() or not partials.is_contiguous():
        raise RuntimeError(f"{who}: partials must be contiguous float32 and bad contiguous int32 GPU tensors")
    if partials.numel() < 4 * int(nchunks) or bad.numel() < 2 * int(nchunks):
        raise RuntimeError(f"{who}: {int(nchunks)} records need four partials and two counts each")


def tensor_stats_stage1(p: Tensor, g: Tensor, chunks: Tensor, nchunks: int, partials: Tensor, bad: Tensor):
    """First pass of the per-tensor statistics (include/ytvln.h: ytvln_tensor_stats_stage1) over an AdamW chunk table, on the current stream:
    partials[4i : 4i+4] = [sum g^2, max |g|, sum p^2, max |p|] over the finite elements of record i and bad[2i : 2i+2] = its non-finite
    elements of g and of p.  `g`: the fp32 gradient arena or the bf16 exchange buffer.  Read-only for p and g."""
    _check(p, "p")
    dt = _grad_dtype(g)
    _check(g, "g", g.dtype)
    _check_stats_partials(partials, bad, nchunks, "tensor_stats_stage1")
    call("ytvln_tensor_stats_stage1", _ptr(p), g.data_ptr(), dt, chunks.data_ptr(), int(nchunks), _ptr(partials), bad.data_ptr(), _stream())


def tensor_stats_stage2(partials: Tensor, bad: Tensor, nchunks: int, tensor_first: Tensor, rec_tensor: Tensor, ntensors: int,
                        grad_scale: float, stats: Tensor, counts: Tensor):
    """stats[k] = [grad_scale * ||g||, grad_scale * max |g|, ||p||, max |p|] and counts[k] = [non-finite g, non-finite p, launches so far
    with a non-finite g] for every tensor of a chunk table from the partials of tensor_stats_stage1 (include/ytvln.h:
    ytvln_tensor_stats_stage2), on the current stream.  `tensor_first` / `rec_tensor` as for lamb_trust; stats (float32, four per row) and
    counts (int64, three per row) are indexed by rec_tensor's values."""
    _check(stats, "stats")
    _check(counts, "counts", torch.int64)
    _check_stats_partials(partials, bad, nchunks, "tensor_stats_stage2")
    _check_i32(tensor_first, "tensor_first", int(ntensors) + 1)
    _check_i32(rec_tensor, "rec_tensor", int(nchunks))
    if not stats.is_contiguous() or not counts.is_contiguous() or stats.numel() % 4 or counts.numel() * 4 != stats.numel() * 3:
        raise RuntimeError("tensor_stats_stage2: stats must hold four floats and counts three int64 per row, both contiguous")
    call("ytvln_tensor_stats_stage2", _ptr(partials), bad.data_ptr(), tensor_first.data_ptr(), rec_tensor.data_ptr(), int(ntensors),
         float(grad_scale), _ptr(stats), counts.data_ptr(), _stream())
