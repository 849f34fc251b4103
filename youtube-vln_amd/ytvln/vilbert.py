"""ViLBERT two-stream co-attentional transformer on hand-written CDNA4 kernels.

Drop-in counterpart of the reference `vilbert/vilbert.py`: the same class names, constructor arguments, `forward`
signatures / return structures and state-dict keys (tests/golden/state_dict_schema.json is dumped from the reference), so
`pretrain.py` / `train.py` / `lily.py` can import these classes instead of the reference's.  The modules only *hold*
parameters (nn.Linear / nn.Embedding containers are created in the reference's order so that seeded initialisation draws
the same numbers); all arithmetic goes through `ytvln.ops` -> libytvln.so:

  reference (vilbert/vilbert.py)                         here
  ------------------------------------------------------ ---------------------------------------------------------------
  BertEmbeddings.forward            :240-256             one fused gather+add+LayerNorm+dropout kernel
  BertImageEmbeddings.forward       :1356-1370           MFMA GEMM (2048->Hv) + one fused loc/orient/frame+LN+dropout kernel
  Bert(Image)SelfAttention.forward  :284-311 / :413-440  one packed QKV GEMM + fused flash attention (scores stay in registers)
  Bert(Image)SelfOutput / *Output   :321-325 / :364-368  GEMM + fused dropout+residual+LayerNorm kernel
  Bert(Image)Intermediate           :351-354             GEMM with erf-GELU epilogue (fused into ops.ffn with the next GEMM)
  BertBiAttention.forward           :552-618             per-direction packed K|V GEMMs + the same attention kernel both ways
  heads                             :851-969             GEMM(+GELU) + LayerNorm kernel + decoder GEMM

GPU only: tensors must be on a HIP device; there is no CPU path (use `oracle/` for CPU checks -- tests only).
"""
from __future__ import annotations

import contextlib
import copy
import json
import logging
import math
import os
import warnings
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
from torch import nn

from . import ops
from .ops import DropoutState

logger = logging.getLogger(__name__)


@dataclass
class BertConfig:
    """Same fields / defaults / strictness as the reference dataclass (vilbert/vilbert.py:129-195)."""
    vocab_size: int = 30522
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    hidden_act: str = "gelu"
    hidden_dropout_prob: float = 0.1
    attention_probs_dropout_prob: float = 0.1
    max_position_embeddings: int = 512
    type_vocab_size: int = 2
    initializer_range: float = 0.02
    v_feature_size: int = 2048
    v_target_size: int = 1601
    v_hidden_size: int = 768
    v_num_hidden_layers: int = 3
    v_num_attention_heads: int = 12
    v_intermediate_size: int = 3072
    bi_hidden_size: int = 1024
    bi_num_attention_heads: int = 16
    v_attention_probs_dropout_prob: float = 0.1
    v_hidden_act: str = "gelu"
    v_hidden_dropout_prob: float = 0.1
    v_initializer_range: float = 0.2
    v_biattention_id: Tuple[int, ...] = (0, 1)
    t_biattention_id: Tuple[int, ...] = (10, 11)
    order_hidden_size: int = 512
    predict_feature: int = False
    fast_mode: int = False
    fixed_v_layer: int = 0
    fixed_t_layer: int = 0
    in_batch_pairs: int = False
    fusion_method: str = "mul"
    intra_gate: int = False
    with_coattention: int = True
    ranking: bool = True
    masked_language: bool = False
    masked_vision: bool = False

    def __post_init__(self):
        assert len(self.v_biattention_id) == len(self.t_biattention_id)
        assert max(self.v_biattention_id) < self.v_num_hidden_layers
        assert max(self.t_biattention_id) < self.num_hidden_layers

    @classmethod
    def from_json_file(cls, json_file):
        with open(json_file, "r", encoding="utf-8") as fid:
            return cls(**json.load(fid))

    def to_dict(self):
        return copy.deepcopy(self.__dict__)

    def to_json_string(self):
        return json.dumps({k: v for k, v in self.to_dict().items() if k != "args"}, indent=2, sort_keys=True, default=str) + "\n"

    def __repr__(self):
        return str(self.to_json_string())


# ------------------------------------------------------------------------------------------------------------------
# per-forward runtime context (dropout key material); set by the outermost model forward
# ------------------------------------------------------------------------------------------------------------------
class _Runtime:
    drop: Optional[DropoutState] = None
    ffn_recompute: bool = False          # BertEncoder.recompute == "ffn", for the duration of that encoder's forward (read by _ffn_block)
    plans = None                         # BertModel.skip_padding: (text RowsPlan | None, image RowsPlan | None) while such a forward, or the
                                         # recomputation of one of its layers, runs; None = every row of both streams is padded (the default)
    live = None                          # (text LiveRows | None, image LiveRows | None) while a training forward of BertModel with padding masks runs


def _live(side: int):
    """Context for the projections of the text (0) / image (1) side: their weight gradients contract over that side's valid rows
    (ops.live_rows_scope) while BertModel has lists installed, a plain pass-through otherwise."""
    live = _Runtime.live
    return contextlib.nullcontext() if live is None or live[side] is None else ops.live_rows_scope(live[side])


class _RowsHint:
    """The host's guess of one side's valid-row count (BertModel.rows_hint).  step(count) returns the guess for this forward and, when not
    capturing, posts `count` (device int32 [1]) for a later one: a non-blocking copy into pinned memory with an event behind it.  A forward that
    finds the event complete takes the value, rounded up to 256 rows; under capture the last value is used and nothing is posted or queried."""

    def __init__(self):
        self.value, self.pinned, self.event = 0, None, None

    def step(self, count) -> int:
        if torch.cuda.is_current_stream_capturing():
            return self.value
        if self.event is not None and self.event.query():
            self.value = -(-int(self.pinned[0]) // 256) * 256
            self.event = None
        if self.event is None:          # (one copy in flight at a time: the pinned word is read only behind its event)
            if self.pinned is None:
                self.pinned = torch.zeros(1, dtype=torch.int32).pin_memory()
            self.pinned.copy_(count, non_blocking=True)
            self.event = torch.cuda.Event()
            self.event.record()
        return self.value


def _plan(side: int):
    """The RowsPlan of the text (0) / image (1) stream when its hidden states are packed rows [1, capacity, H], else None."""
    return None if _Runtime.plans is None else _Runtime.plans[side]


def _with_plans(plans, fn, *args):
    """fn(*args) with `plans` installed: a recomputed layer runs in the backward pass, long after its forward's plans were taken down."""
    prev, _Runtime.plans = _Runtime.plans, plans
    try:
        return fn(*args)
    finally:
        _Runtime.plans = prev


SKIP_PADDING_TILE = 256          # packed capacities are whole 256-row GEMM tiles


def _skip_padding_spec(value):
    """BertModel.skip_padding, validated -> None or a (text, image) pair whose entries are "exact" or a fraction in (0, 1]."""
    def one(v):
        if isinstance(v, str):
            return v == "exact"
        return isinstance(v, (int, float)) and not isinstance(v, bool) and 0.0 < float(v) <= 1.0
    if value is None:
        return None
    if one(value):
        return (value, value)
    if isinstance(value, (tuple, list)) and len(value) == 2 and all(one(v) and not isinstance(v, str) for v in value):
        return (value[0], value[1])
    raise ValueError(f"BertModel.skip_padding = {value!r}: expected None, a fraction in (0, 1], a (text, image) pair of such fractions, or \"exact\"")


def _side_plan(mask, spec):
    """RowsPlan of one padding mask [N, L] (non-zero = valid).  A fraction: static capacity, no host sync, capturable.  "exact": the count is read
    on the host (one sync) and rounded up to a whole tile."""
    rows = mask.numel()
    if spec == "exact":
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('BertModel.skip_padding = "exact" reads the number of valid rows on the host and cannot be captured into a graph; '
                               "give a static capacity (a fraction in (0, 1])")
        count = int((mask != 0).sum())
        cap = min(rows, max(1, -(-count // SKIP_PADDING_TILE)) * SKIP_PADDING_TILE)
    else:
        cap = ops.rows_capacity(rows, spec)
    return ops.rows_plan(mask, cap)


def _begin_forward(module: nn.Module, device) -> None:
    _Runtime.drop = DropoutState(device) if module.training else None


def _drop_state(module: nn.Module, x: torch.Tensor) -> Optional[DropoutState]:
    if not module.training:
        return None
    if _Runtime.drop is None:
        # (a module used on its own, e.g. a bare BertEncoder: no _begin_forward ran.)  Inside a two-stream region the clone of the seed and the
        # counter increment must be ordered before BOTH sides' first read: enqueue them on the main stream and make that the new fork point,
        # whichever side asks first (created on the side stream, the main stream could read the state before it was written).
        with ops.TwoStream.shared_write():
            _Runtime.drop = DropoutState(x.device)
        _share_drop_state()
    return _Runtime.drop


def _share_drop_state() -> None:
    """Inside a two-stream region the (seed, counter) tensor of this forward is read by kernels of both HIP streams."""
    ts = ops.TwoStream
    if ts.active and _Runtime.drop is not None:
        t = _Runtime.drop.tensor
        t.record_stream(ts.side_stream(t.device))
        if ts.main is not None:
            t.record_stream(ts.main)


# ------------------------------------------------------------------------------------------------------------------
# activation recomputation (BertEncoder.recompute): opt-in, bit-exact
# ------------------------------------------------------------------------------------------------------------------
RECOMPUTE_TIERS = ("none", "ffn", "layer")


@contextlib.contextmanager
def _replay_drop(state, site: int):
    """Install `state` -- the DropoutState OBJECT a segment recorded when it first ran -- as _Runtime.drop with its site counter rewound to
    `site`, the counter's value on entry to that first run: the body then asks for the same (rng tensor, site) pairs in the same order and
    every dropout kernel draws the masks of the forward.  Whatever was installed before comes back afterwards, and so does the counter, also
    when the body raises.  The recorded object is used, never the _Runtime.drop of the moment: by the time a backward pass recomputes,
    another forward (a second model, the next micro-step) may have replaced it."""
    prev = _Runtime.drop
    back = None if state is None else state._site
    if state is not None:
        state._site = int(site)
    _Runtime.drop = state
    try:
        yield state
    finally:
        _Runtime.drop = prev
        if state is not None:
            state._site = back


class _RecomputeLayerFn(torch.autograd.Function):
    """One encoder layer (text, image or connection) as ONE autograd node that keeps only its inputs (recompute = "layer").

    forward: runs `fn(*hidden, *rest)` with gradients off (a Function's forward always does) -- the same launches on the same inputs as the
    plain layer, and the dropout site counter advances exactly as it does there, so every site after the layer keeps its id.  It records the
    DropoutState object of this forward and the counter's value on entry.
    backward: re-runs `fn` with gradients on under _replay_drop (same kernels, same inputs, same masks: the same bits), then sends the incoming
    gradients through that sub-graph.  Parameter gradients are accumulated by the inner backward itself (arena-direct writes happen once,
    there; post-accumulate hooks fire from there, once); the node returns the gradients of the hidden states only.  The parameters are NOT
    inputs of the node (their AccumulateGrad nodes would run a second time from the outer graph and fire every hook twice); `anchor`, an
    empty leaf that requires a gradient and never gets one, is: the node then takes part in a backward pass whose hidden states carry no
    gradient (a frozen prefix below it).
    The recomputation runs on the stream the engine gives the node -- the stream of its forward -- with two-stream mode off: a connection
    layer, which spans both sides, is recomputed on one stream (bit-identical, see ops.TwoStream)."""

    @staticmethod
    def forward(ctx, fn, n_hidden, anchor, *tensors):
        ctx.set_materialize_grads(False)
        ctx.fn, ctx.n_hidden = fn, n_hidden
        st = _Runtime.drop
        ctx.site = st._site if st is not None else 0
        out = fn(*tensors)
        ctx.drop = st if st is not None else _Runtime.drop          # (a bare encoder: the state is created by the first dropout site, counter 0)
        ctx.is_tensor = [torch.is_tensor(t) for t in tensors]
        ctx.other = [None if torch.is_tensor(t) else t for t in tensors]
        ctx.save_for_backward(*[t for t in tensors if torch.is_tensor(t)])
        return out

    @staticmethod
    def backward(ctx, *grads):
        it = iter(ctx.saved_tensors)
        tensors = [next(it) if is_t else o for is_t, o in zip(ctx.is_tensor, ctx.other)]
        cur = torch.cuda.current_stream()
        for t in tensors:          # a connection layer reads, on this stream, hidden states the other stream produced
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(cur)
        hidden = [t.detach().requires_grad_(ctx.needs_input_grad[3 + i]) for i, t in enumerate(tensors[:ctx.n_hidden])]
        ts = ops.TwoStream
        was_active, ts.active = ts.active, False
        try:
            with torch.enable_grad(), _replay_drop(ctx.drop, ctx.site):
                out = ctx.fn(*hidden, *tensors[ctx.n_hidden:])
        finally:
            ts.active = was_active
        out = out if isinstance(out, tuple) else (out,)
        pairs = [(o, g) for o, g in zip(out, grads) if g is not None and o.requires_grad]
        if pairs:
            torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
        return (None, None, None) + tuple(h.grad for h in hidden) + (None,) * (len(ctx.needs_input_grad) - 3 - ctx.n_hidden)


def _recompute_layer(fn, hidden, rest):
    """`fn(*hidden, *rest)` -> a tensor or a tuple of tensors, as one recomputed node.  `hidden`: the hidden states (differentiated);
    `rest`: masks and flags (not differentiated)."""
    anchor = torch.empty(0, device=hidden[0].device, requires_grad=True)
    return _RecomputeLayerFn.apply(fn, len(hidden), anchor, *hidden, *rest)


def _p(module: nn.Module, p: float) -> float:
    return float(p) if module.training else 0.0


def gelu(x: torch.Tensor) -> torch.Tensor:
    """vilbert.py:113-119: the exact (erf) GELU.  Inside the model the activation is fused into the GEMM epilogue (ops.linear(..., "gelu"));
    this stand-alone form exists for callers that import it."""
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def swish(x: torch.Tensor) -> torch.Tensor:
    """vilbert.py:122-123."""
    return x * torch.sigmoid(x)


ACT2FN = {"gelu": gelu, "relu": torch.nn.functional.relu, "swish": swish}        # vilbert.py:126


def load_tf_weights_in_bert(model, tf_checkpoint_path):
    """vilbert.py:58-110 reads a TensorFlow checkpoint through the `tensorflow` package.  Not part of the hot path and not available
    here: convert the checkpoint to a PyTorch state dict once (the reference's own loader does that) and use `from_pretrained`."""
    raise NotImplementedError("TensorFlow checkpoints are not read by this build; convert to a PyTorch state dict and use from_pretrained()")


def _act_name(act) -> str:
    if not isinstance(act, str) or act not in ("gelu", "relu", "swish"):
        raise NotImplementedError(f"activation {act!r}: the HIP path implements the strings 'gelu' (erf form), 'relu' and 'swish' "
                                  "(callables and other names are refused)")
    return act


def _mask2d(mask: torch.Tensor, n: int, t: int) -> torch.Tensor:
    """Additive attention mask as [N, T] fp32.  The reference passes it extended to [N,1,1,T] (vilbert.py:1268-1287)."""
    if mask.numel() != n * t:
        raise NotImplementedError(f"attention mask of shape {tuple(mask.shape)}: only per-key masks ([N,1,1,T]) are supported")
    m = mask.reshape(n, t)
    if m.dtype != torch.float32:
        m = m.float()
    return m.contiguous()


def _self_mask(mask: torch.Tensor, n: int, t: int, heads: int):
    """(per-key mask [N, T] or None, per-score bias or None) of a self-attention `attention_mask`.  N*T elements: the per-key path, exactly as
    before.  [N,1,T,T], [N,heads,T,T] and [1,1,T,T] -- anything else the reference's `attention_scores + attention_mask` broadcast
    (vilbert.py:294-297, 423-427) would take is refused -- go to the kernels' bias operand, read in place, with no key mask."""
    if mask.numel() == n * t and (mask.dim() != 4 or mask.shape[2] == 1):
        return _mask2d(mask, n, t), None
    if mask.dim() == 4 and tuple(mask.shape[2:]) == (t, t) and mask.shape[0] in (1, n) and mask.shape[1] in (1, heads) \
            and (mask.shape[0] == n or mask.shape[1] == 1):
        return None, mask
    raise NotImplementedError(f"attention mask of shape {tuple(mask.shape)}: accepted are per-key masks of N*T elements ([N,1,1,T]) and "
                              f"per-score masks [N,1,T,T], [N,heads,T,T], [1,1,T,T] (N {n}, heads {heads}, T {t})")


class BertLayerNorm(nn.Module):
    """TF-style LayerNorm, eps inside the sqrt (vilbert.py:204-217) -- fused kernel."""

    def __init__(self, hidden_size, eps=1e-12):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden_size))
        self.bias = nn.Parameter(torch.zeros(hidden_size))
        self.variance_epsilon = eps

    def forward(self, x):
        return ops.add_layer_norm(x, None, self.weight, self.bias, self.variance_epsilon)


def _add_ln(ln: BertLayerNorm, x, res, module, p_pre=0.0, p_post=0.0):
    return ops.add_layer_norm(x, res, ln.weight, ln.bias, ln.variance_epsilon, _p(module, p_pre), _p(module, p_post),
                              _drop_state(module, x))


class BertEmbeddings(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.word_embeddings = nn.Embedding(config.vocab_size, config.hidden_size, padding_idx=0)
        self.position_embeddings = nn.Embedding(config.max_position_embeddings, config.hidden_size)
        self.token_type_embeddings = nn.Embedding(config.type_vocab_size, config.hidden_size)
        self.LayerNorm = BertLayerNorm(config.hidden_size, eps=1e-12)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)

    def forward(self, input_ids, token_type_ids=None):
        return ops.text_embed(input_ids, token_type_ids, self.word_embeddings.weight, self.position_embeddings.weight,
                              self.token_type_embeddings.weight, self.LayerNorm.weight, self.LayerNorm.bias,
                              self.LayerNorm.variance_epsilon, _p(self, self.dropout.p), _drop_state(self, self.LayerNorm.weight))


class _PackedQKV:
    """Helper: one [3H, Hin] projection instead of three (the reference runs query/key/value as separate Linears)."""

    @staticmethod
    def project(x, q: nn.Linear, k: nn.Linear, v: nn.Linear):
        return ops.linear(x, ops.pack_rows(q.weight, k.weight, v.weight), ops.pack_rows(q.bias, k.bias, v.bias))

    @staticmethod
    def project_res(x, q: nn.Linear, k: nn.Linear, v: nn.Linear):
        """(q|k|v projection, x for the residual around the attention block): see ops.LinearFn(passthrough)."""
        return ops.linear_res(x, ops.pack_rows(q.weight, k.weight, v.weight), ops.pack_rows(q.bias, k.bias, v.bias))


class _SelfAttentionBase(nn.Module):
    """Shared forward of BertSelfAttention / BertImageSelfAttention."""

    want_probs = False
    _side = 0          # the stream whose RowsPlan (BertModel.skip_padding) this site reads: 0 text, 1 image

    def _build(self, hidden, heads, p_attn):
        if hidden % heads != 0:
            raise ValueError("The hidden size (%d) is not a multiple of the number of attention heads (%d)" % (hidden, heads))
        self.num_attention_heads = heads
        self.attention_head_size = int(hidden / heads)
        self.all_head_size = self.num_attention_heads * self.attention_head_size
        self.query = nn.Linear(hidden, self.all_head_size)
        self.key = nn.Linear(hidden, self.all_head_size)
        self.value = nn.Linear(hidden, self.all_head_size)
        self.dropout = nn.Dropout(p_attn)

    def forward(self, hidden_states, attention_mask):
        out, probs, _ = self.forward_res(hidden_states, attention_mask)
        return out, probs

    def forward_res(self, hidden_states, attention_mask):
        """(context, probs, hidden_states-for-the-residual): the third value is what the caller's `LayerNorm(dense(context) + input)`
        must use as `input` so that the two gradients of `hidden_states` meet inside the projection's input-gradient GEMM."""
        plan = _plan(self._side)
        if plan is None:
            n, t, _ = hidden_states.shape
        else:          # packed rows [1, capacity, H]: the mask carries the padded geometry
            t = attention_mask.shape[-1]
            n = plan.rows // t
        mask, bias = _self_mask(attention_mask, n, t, self.num_attention_heads)
        qkv, residual = _PackedQKV.project_res(hidden_states, self.query, self.key, self.value)
        if plan is None:
            qkv = qkv.view(n * t, 3 * self.all_head_size)
        else:          # the attention kernels read the padded [N*T, 3H] layout: masks, biases, dropout and probabilities keep padded coordinates
            qkv = ops.rows_unpack(qkv.view(plan.capacity, 3 * self.all_head_size), plan)
        p = _p(self, self.dropout.p)
        st = _drop_state(self, qkv) if p > 0 else None
        extra = () if bias is None else (bias,)          # (no bias: the call, and the launch behind it, as it always was)
        if bias is not None and bias.is_cuda and ops.TwoStream.active:
            bias.record_stream(torch.cuda.current_stream())          # the text layers run on the side stream: a full mask made on the main one is read there
        out, lse = ops.SelfAttentionFn.apply(qkv, mask, n, t, self.num_attention_heads, p, st.tensor if st else None,
                                             st.next_site() if st else 0, *extra)
        probs = None
        if self.want_probs:
            with torch.no_grad():
                h = self.all_head_size
                probs = ops.attn_probs(qkv, 0, 3 * h, qkv, h, 3 * h, mask, lse, n, self.num_attention_heads, t, t,
                                       self.attention_head_size, 1.0 / math.sqrt(self.attention_head_size), bias=bias)
        if plan is not None:
            return ops.rows_pack(out, plan).view(1, plan.capacity, self.all_head_size), probs, residual
        return out.view(n, t, self.all_head_size), probs, residual


class BertSelfAttention(_SelfAttentionBase):
    def __init__(self, config):
        super().__init__()
        self._build(config.hidden_size, config.num_attention_heads, config.attention_probs_dropout_prob)


class _SelfOutputBase(nn.Module):
    def _build(self, hidden, p):
        self.dense = nn.Linear(hidden, hidden)
        self.LayerNorm = BertLayerNorm(hidden, eps=1e-12)
        self.dropout = nn.Dropout(p)

    def forward(self, hidden_states, input_tensor):
        h = ops.linear(hidden_states, self.dense.weight, self.dense.bias)
        return _add_ln(self.LayerNorm, h, input_tensor, self, p_pre=self.dropout.p)


class BertSelfOutput(_SelfOutputBase):
    def __init__(self, config):
        super().__init__()
        self._build(config.hidden_size, config.hidden_dropout_prob)


class BertAttention(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.self = BertSelfAttention(config)
        self.output = BertSelfOutput(config)

    def forward(self, input_tensor, attention_mask):
        self_output, attention_probs, residual = self.self.forward_res(input_tensor, attention_mask)
        return self.output(self_output, residual), attention_probs


class _IntermediateBase(nn.Module):
    def _build(self, hidden, inter, act):
        self.dense = nn.Linear(hidden, inter)
        self.intermediate_act_fn = act

    def forward(self, hidden_states):
        return ops.linear(hidden_states, self.dense.weight, self.dense.bias, _act_name(self.intermediate_act_fn))


class BertIntermediate(_IntermediateBase):
    def __init__(self, config):
        super().__init__()
        self._build(config.hidden_size, config.intermediate_size, config.hidden_act)


class _OutputBase(nn.Module):
    def _build(self, inter, hidden, p):
        self.dense = nn.Linear(inter, hidden)
        self.LayerNorm = BertLayerNorm(hidden, eps=1e-12)
        self.dropout = nn.Dropout(p)

    def forward(self, hidden_states, input_tensor):
        h = ops.linear(hidden_states, self.dense.weight, self.dense.bias)
        return _add_ln(self.LayerNorm, h, input_tensor, self, p_pre=self.dropout.p)


class BertOutput(_OutputBase):
    def __init__(self, config):
        super().__init__()
        self._build(config.intermediate_size, config.hidden_size, config.hidden_dropout_prob)


def _ffn_block(inter: _IntermediateBase, out: _OutputBase, x):
    """intermediate -> output of a layer, with the two GEMMs and the GELU fused in one autograd node when possible."""
    if _act_name(inter.intermediate_act_fn) == "gelu":
        if _Runtime.ffn_recompute:          # recompute = "ffn": keep z, rebuild h = gelu(z) in the backward (fp32 only: bf16 hidden states raise)
            h, residual = ops.ffn_res(x, inter.dense.weight, inter.dense.bias, out.dense.weight, out.dense.bias, recompute_h=True)
        else:
            h, residual = ops.ffn_res(x, inter.dense.weight, inter.dense.bias, out.dense.weight, out.dense.bias)
        return _add_ln(out.LayerNorm, h, residual, out, p_pre=out.dropout.p)
    return out(inter(x), x)


class BertLayer(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.attention = BertAttention(config)
        self.intermediate = BertIntermediate(config)
        self.output = BertOutput(config)

    def forward(self, hidden_states, attention_mask):
        attention_output, attention_probs = self.attention(hidden_states, attention_mask)
        return _ffn_block(self.intermediate, self.output, attention_output), attention_probs


class BertImageSelfAttention(_SelfAttentionBase):
    _side = 1

    def __init__(self, config):
        super().__init__()
        self._build(config.v_hidden_size, config.v_num_attention_heads, config.v_attention_probs_dropout_prob)


class BertImageSelfOutput(_SelfOutputBase):
    def __init__(self, config):
        super().__init__()
        self._build(config.v_hidden_size, config.v_hidden_dropout_prob)


class BertImageAttention(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.self = BertImageSelfAttention(config)
        self.output = BertImageSelfOutput(config)

    def forward(self, input_tensor, attention_mask):
        self_output, attention_probs, residual = self.self.forward_res(input_tensor, attention_mask)
        return self.output(self_output, residual), attention_probs


class BertImageIntermediate(_IntermediateBase):
    def __init__(self, config):
        super().__init__()
        self._build(config.v_hidden_size, config.v_intermediate_size, config.v_hidden_act)


class BertImageOutput(_OutputBase):
    def __init__(self, config):
        super().__init__()
        self._build(config.v_intermediate_size, config.v_hidden_size, config.v_hidden_dropout_prob)


class BertImageLayer(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.attention = BertImageAttention(config)
        self.intermediate = BertImageIntermediate(config)
        self.output = BertImageOutput(config)

    def forward(self, hidden_states, attention_mask):
        attention_output, attention_probs = self.attention(hidden_states, attention_mask)
        return _ffn_block(self.intermediate, self.output, attention_output), attention_probs


class BertBiAttention(nn.Module):
    """Cross-stream co-attention (vilbert.py:512-618).  stream 1 = vision, stream 2 = text."""

    want_probs = False

    def __init__(self, config):
        super().__init__()
        if config.bi_hidden_size % config.bi_num_attention_heads != 0:
            raise ValueError("The hidden size (%d) is not a multiple of the number of attention heads (%d)"
                             % (config.bi_hidden_size, config.bi_num_attention_heads))
        self.num_attention_heads = config.bi_num_attention_heads
        self.attention_head_size = int(config.bi_hidden_size / config.bi_num_attention_heads)
        self.all_head_size = self.num_attention_heads * self.attention_head_size
        self.query1 = nn.Linear(config.v_hidden_size, self.all_head_size)
        self.key1 = nn.Linear(config.v_hidden_size, self.all_head_size)
        self.value1 = nn.Linear(config.v_hidden_size, self.all_head_size)
        self.dropout1 = nn.Dropout(config.v_attention_probs_dropout_prob)
        self.query2 = nn.Linear(config.hidden_size, self.all_head_size)
        self.key2 = nn.Linear(config.hidden_size, self.all_head_size)
        self.value2 = nn.Linear(config.hidden_size, self.all_head_size)
        self.dropout2 = nn.Dropout(config.attention_probs_dropout_prob)

    def forward(self, input_tensor1, attention_mask1, input_tensor2, attention_mask2, co_attention_mask=None,
                use_co_attention_mask=False):
        """The reference's 3-tuple (vilbert.py:618)."""
        return self.forward_res(input_tensor1, attention_mask1, input_tensor2, attention_mask2, co_attention_mask, use_co_attention_mask)[:3]

    def forward_res(self, input_tensor1, attention_mask1, input_tensor2, attention_mask2, co_attention_mask=None,
                    use_co_attention_mask=False):
        """forward() plus the two stream inputs as they leave the projections' autograd nodes (the residual values BertBiOutput adds):
        returned, not parked on the module -- no graph stays pinned between calls and a direct forward() cannot leave a stale pair behind
        (ADVICE r2).  BertConnectionLayer calls this form."""
        plan_t, plan_v = _plan(0), _plan(1)
        if plan_v is None:
            n, r, _ = input_tensor1.shape
        else:          # packed rows: the masks carry the padded geometry
            r = attention_mask1.shape[-1]
            n = plan_v.rows // r
        t = input_tensor2.shape[1] if plan_t is None else attention_mask2.shape[-1]
        hb = self.all_head_size
        # use_co_attention_mask (vilbert.py:581-582, 603-604): co_attention_mask [N,1,R,T] is added to the scores of regions over tokens as it is
        # and to those of tokens over regions through its transposed VIEW (the kernels read it through swapped strides: no copy)
        bias1 = bias2 = None
        if use_co_attention_mask:
            if co_attention_mask is None or co_attention_mask.dim() != 4 or tuple(co_attention_mask.shape[2:]) != (r, t):
                raise NotImplementedError("use_co_attention_mask=True needs a co_attention_mask of shape [N,1,R,T] (or [N,heads,R,T], [1,1,R,T]), got "
                                          f"{None if co_attention_mask is None else tuple(co_attention_mask.shape)}")
            bias2 = co_attention_mask if co_attention_mask.dtype == torch.float32 else co_attention_mask.float()
            bias1 = bias2.transpose(2, 3)
        m1, m2 = _mask2d(attention_mask1, n, r), _mask2d(attention_mask2, n, t)
        # each stream's input feeds two projections and the residual of BertBiOutput: the residual value travels through both
        # projections' autograd nodes (ops.LinearFn passthrough) so the three gradients meet inside the input-gradient GEMMs
        with _live(1):
            q1, res1 = ops.linear_res(input_tensor1, self.query1.weight, self.query1.bias)
            kv1, res1 = ops.linear_res(res1, ops.pack_rows(self.key1.weight, self.value1.weight), ops.pack_rows(self.key1.bias, self.value1.bias))
        if plan_v is not None:
            q1, kv1 = ops.rows_unpack(q1.view(-1, hb), plan_v), ops.rows_unpack(kv1.view(-1, 2 * hb), plan_v)
        with ops.TwoStream.side(input_tensor2), _live(0):         # the text side's projections: second HIP stream when two-stream mode is on
            q2, res2 = ops.linear_res(input_tensor2, self.query2.weight, self.query2.bias)
            kv2, res2 = ops.linear_res(res2, ops.pack_rows(self.key2.weight, self.value2.weight), ops.pack_rows(self.key2.bias, self.value2.bias))
            if plan_t is not None:
                q2, kv2 = ops.rows_unpack(q2.view(-1, hb), plan_t), ops.rows_unpack(kv2.view(-1, 2 * hb), plan_t)
        ops.TwoStream.join(q2, kv2)
        q1, kv1, q2, kv2 = q1.view(n * r, hb), kv1.view(n * r, 2 * hb), q2.view(n * t, hb), kv2.view(n * t, 2 * hb)
        p1, p2 = _p(self, self.dropout1.p), _p(self, self.dropout2.p)
        st = _drop_state(self, q1) if (p1 > 0 or p2 > 0) else None
        s1, s2 = (st.next_site(), st.next_site()) if st else (0, 0)
        extra = () if bias2 is None else (bias1, bias2)
        ctx1, ctx2, lse1, lse2 = ops.CoAttentionFn.apply(q1, kv1, q2, kv2, m1, m2, n, r, t, self.num_attention_heads, p1, p2,
                                                         st.tensor if st else None, s1, s2, *extra)
        out1 = ctx1.view(n, t, hb) if plan_t is None else ops.rows_pack(ctx1, plan_t).view(1, plan_t.capacity, hb)
        out2 = ctx2.view(n, r, hb) if plan_v is None else ops.rows_pack(ctx2, plan_v).view(1, plan_v.capacity, hb)
        ops.TwoStream.mark()                            # both context tensors exist: the text side may go on from here
        probs = (None, None)
        if self.want_probs:
            with torch.no_grad():
                sc = 1.0 / math.sqrt(self.attention_head_size)
                pr1 = ops.attn_probs(q2, 0, hb, kv1, 0, 2 * hb, m1, lse1, n, self.num_attention_heads, t, r,
                                     self.attention_head_size, sc, bias=bias1)
                pr2 = ops.attn_probs(q1, 0, hb, kv2, 0, 2 * hb, m2, lse2, n, self.num_attention_heads, r, t,
                                     self.attention_head_size, sc, bias=bias2)
                probs = (pr1, pr2)
        return out1, out2, probs, res1, res2


class BertBiOutput(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.dense1 = nn.Linear(config.bi_hidden_size, config.v_hidden_size)
        self.LayerNorm1 = BertLayerNorm(config.v_hidden_size, eps=1e-12)
        self.dropout1 = nn.Dropout(config.v_hidden_dropout_prob)
        self.q_dense1 = nn.Linear(config.bi_hidden_size, config.v_hidden_size)   # declared, never used (vilbert.py:628)
        self.q_dropout1 = nn.Dropout(config.v_hidden_dropout_prob)
        self.dense2 = nn.Linear(config.bi_hidden_size, config.hidden_size)
        self.LayerNorm2 = BertLayerNorm(config.hidden_size, eps=1e-12)
        self.dropout2 = nn.Dropout(config.hidden_dropout_prob)
        self.q_dense2 = nn.Linear(config.bi_hidden_size, config.hidden_size)     # declared, never used (vilbert.py:635)
        self.q_dropout2 = nn.Dropout(config.hidden_dropout_prob)

    def forward(self, hidden_states1, input_tensor1, hidden_states2, input_tensor2):
        with _live(1):
            c1 = ops.linear(hidden_states1, self.dense1.weight, self.dense1.bias)
        with ops.TwoStream.side(hidden_states2, input_tensor2), _live(0):
            c2 = ops.linear(hidden_states2, self.dense2.weight, self.dense2.bias)
        h1 = _add_ln(self.LayerNorm1, c1, input_tensor1, self, p_pre=self.dropout1.p)
        with ops.TwoStream.side():
            h2 = _add_ln(self.LayerNorm2, c2, input_tensor2, self, p_pre=self.dropout2.p)
        return h1, h2


class BertConnectionLayer(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.biattention = BertBiAttention(config)
        self.biOutput = BertBiOutput(config)
        self.v_intermediate = BertImageIntermediate(config)
        self.v_output = BertImageOutput(config)
        self.t_intermediate = BertIntermediate(config)
        self.t_output = BertOutput(config)

    def forward(self, input_tensor1, attention_mask1, input_tensor2, attention_mask2, co_attention_mask=None,
                use_co_attention_mask=False):
        bi_output1, bi_output2, co_attention_probs, res1, res2 = self.biattention.forward_res(
            input_tensor1, attention_mask1, input_tensor2, attention_mask2, co_attention_mask, use_co_attention_mask)
        # bi_output2 (image queries over text) feeds the vision stream, bi_output1 the text stream (vilbert.py:671)
        attention_output1, attention_output2 = self.biOutput(bi_output2, res1, bi_output1, res2)
        with _live(1):
            layer_output1 = _ffn_block(self.v_intermediate, self.v_output, attention_output1)
        with ops.TwoStream.side(), _live(0):
            layer_output2 = _ffn_block(self.t_intermediate, self.t_output, attention_output2)
        return layer_output1, layer_output2, co_attention_probs


class BertEncoder(nn.Module):
    # Extension (not a BertConfig field: the config stays the reference's strict dataclass).  The reference hard-codes this switch to False as a
    # local of its forward (vilbert.py:736), and False -- parity with it -- is the default here.  Set `encoder.use_co_attention_mask = True` to
    # hand `co_attention_mask` to every connection layer (BertBiAttention adds it to the scores, vilbert.py:581-582, 603-604).
    use_co_attention_mask = False
    # Extension, opt-in (same standing as the switch above: a plain attribute, not a config field): activation recomputation.
    #   "none"   every activation the backward needs is kept (default: nothing changes).
    #   "ffn"    the fused FFN nodes keep the GELU pre-activation z and rebuild h = gelu(z) in their backward with ytvln_gelu_fwd_f32:
    #            rows x intermediate x 4 bytes less per FFN, one elementwise launch more.  fp32 hidden states with "gelu"; "relu" and "swish"
    #            layers are accepted and unchanged (relu keeps only its output; swish is out of scope); bf16 hidden states raise.
    #   "layer"  every text, image and connection layer that runs with gradients becomes one autograd node that keeps only its inputs and
    #            re-runs the layer in the backward, with the dropout masks of the forward replayed from the recorded (DropoutState, site).
    # Losses, gradients and updated parameters are bit-identical to "none" in every tier.  Inert in eval mode and under torch.no_grad().
    recompute = "none"

    def __init__(self, config):
        super().__init__()
        self.FAST_MODE = config.fast_mode
        self.with_coattention = config.with_coattention
        self.v_biattention_id = config.v_biattention_id
        self.t_biattention_id = config.t_biattention_id
        self.in_batch_pairs = config.in_batch_pairs
        self.fixed_t_layer = config.fixed_t_layer
        self.fixed_v_layer = config.fixed_v_layer
        layer = BertLayer(config)
        v_layer = BertImageLayer(config)
        connect_layer = BertConnectionLayer(config)
        self.layer = nn.ModuleList([copy.deepcopy(layer) for _ in range(config.num_hidden_layers)])
        self.v_layer = nn.ModuleList([copy.deepcopy(v_layer) for _ in range(config.v_num_hidden_layers)])
        self.c_layer = nn.ModuleList([copy.deepcopy(connect_layer) for _ in range(len(config.v_biattention_id))])
        # Autograd cut points for a backward pass that runs in phases (ytvln.distributed.GraphedTrainStep, mode "phased": the gradients
        # of the layers above a cut are exchanged between the ranks while the layers below it are still running their backward).
        # Names: "t<i>" / "v<i>" = after text / image layer i, "c<i>" = after co-attention layer i.  At a cut the hidden states are
        # replaced by detached leaves; `_cuts` keeps (outputs below the cut, leaves above it) in forward order.  Values are unchanged.
        self.cut_after = frozenset()
        self._cuts = []

    def _cut(self, name, *hidden):
        if name not in self.cut_after or not torch.is_grad_enabled() or not any(h.requires_grad for h in hidden):
            return hidden if len(hidden) > 1 else hidden[0]
        below = [h for h in hidden if h.requires_grad]
        above = [h.detach().requires_grad_() for h in below]
        self._cuts.append((name, below, above))
        it = iter(above)
        out = tuple(next(it) if h.requires_grad else h for h in hidden)
        return out if len(out) > 1 else out[0]

    def _set_probs(self, flag: bool):
        for m in self.modules():
            if isinstance(m, (_SelfAttentionBase, BertBiAttention)):
                m.want_probs = flag

    def forward(self, txt_embedding, image_embedding, txt_attention_mask, image_attention_mask, co_attention_mask=None,
                output_all_encoded_layers=True, output_all_attention_masks=False):
        """Interleaving schedule of vilbert.py:737-811: for each (v_id, t_id) pair run the pending image layers, the
        pending text layers, then co-attention layer `count`; finally the remaining layers of both streams."""
        tier = self._recompute_tier(output_all_attention_masks)
        self._set_probs(bool(output_all_attention_masks))
        ts = ops.TwoStream
        if self.in_batch_pairs or self.FAST_MODE:
            ts.end(txt_embedding)                        # these modes rebuild the text rows from the image batch: one stream
        else:
            ts.begin(txt_embedding.device)               # (no-op when BertModel.forward opened the region or the mode is off)
        was_ffn, _Runtime.ffn_recompute = _Runtime.ffn_recompute, tier == "ffn"
        try:
            return self._forward(txt_embedding, image_embedding, txt_attention_mask, image_attention_mask, co_attention_mask,
                                 output_all_encoded_layers, output_all_attention_masks, tier == "layer")
        finally:
            ts.active = False
            _Runtime.ffn_recompute = was_ffn

    def _recompute_tier(self, output_all_attention_masks) -> str:
        """The tier this forward runs with: `recompute`, validated, or "none" where the setting is inert (eval mode, gradients off)."""
        tier = self.recompute
        if tier not in RECOMPUTE_TIERS:
            raise ValueError(f"BertEncoder.recompute = {tier!r}: expected one of {RECOMPUTE_TIERS}")
        if tier == "none" or not self.training or not torch.is_grad_enabled():
            return "none"
        if self.cut_after:
            raise NotImplementedError(f"BertEncoder.recompute = {tier!r} with autograd cut points (encoder.cut_after, the phased graph-replayed "
                                      'step): a recomputing backward is not captured; run it with recompute = "none"')
        if tier == "layer" and output_all_attention_masks:
            raise NotImplementedError('BertEncoder.recompute = "layer" with output_all_attention_masks=True: the attention probabilities are an '
                                      'inspection output the recomputed node does not return; run it with recompute = "none"')
        return tier

    def _forward(self, txt_embedding, image_embedding, txt_attention_mask, image_attention_mask, co_attention_mask,
                 output_all_encoded_layers, output_all_attention_masks, recompute_layers=False):
        ts = ops.TwoStream
        v_start = t_start = 0
        all_t, all_v, att_t, att_v, att_c = [], [], [], [], []
        self._cuts = []
        cuts = bool(self.cut_after) and not (self.in_batch_pairs or self.FAST_MODE)

        def run(layers, lo, hi, x, mask, sink, frozen_to, tag):
            for idx in range(lo, hi):
                if idx < frozen_to:
                    with torch.no_grad():
                        x, pr = layers[idx](x, mask)
                elif recompute_layers:
                    # (a trainable per-score mask is differentiated like the hidden states; a constant one is carried along)
                    x, pr = _recompute_layer(lambda h, m, layer=layers[idx], plans=_Runtime.plans: _with_plans(plans, layer, h, m)[0],
                                             *(((x, mask), ()) if mask.requires_grad else ((x,), (mask,)))), None
                else:
                    x, pr = layers[idx](x, mask)
                if cuts:
                    x = self._cut(f"{tag}{idx}", x)
                if output_all_attention_masks:
                    sink.append(pr)
            return x

        for count, (v_end, t_end) in enumerate(zip(self.v_biattention_id, self.t_biattention_id)):
            assert self.fixed_t_layer <= t_end and self.fixed_v_layer <= v_end
            with _live(1):
                image_embedding = run(self.v_layer, v_start, v_end, image_embedding, image_attention_mask, att_v, self.fixed_v_layer, "v")
            with ts.side(txt_embedding, txt_attention_mask), _live(0):
                txt_embedding = run(self.layer, t_start, t_end, txt_embedding, txt_attention_mask, att_t, self.fixed_t_layer, "t")
            if count == 0 and self.in_batch_pairs:
                # every text of the batch against every image of the batch: B -> B^2 rows (vilbert.py:771-778); row (i, j) = text i, image j
                b, r_, hv = image_embedding.shape
                t_, ht = txt_embedding.shape[1], txt_embedding.shape[2]
                image_embedding = image_embedding.unsqueeze(0).expand(b, b, r_, hv).contiguous().view(b * b, r_, hv)
                image_attention_mask = image_attention_mask.reshape(b, -1).unsqueeze(0).expand(b, b, r_).contiguous().view(b * b, 1, 1, r_)
                txt_embedding = txt_embedding.unsqueeze(1).expand(b, b, t_, ht).contiguous().view(b * b, t_, ht)
                txt_attention_mask = txt_attention_mask.reshape(b, -1).unsqueeze(1).expand(b, b, t_).contiguous().view(b * b, 1, 1, t_)
                if self.use_co_attention_mask and co_attention_mask is not None:          # row (i, j) takes text i's mask (vilbert.py:778)
                    co_attention_mask = co_attention_mask.unsqueeze(1).expand(b, b, 1, r_, t_).contiguous().view(b * b, 1, r_, t_)
            if count == 0 and self.FAST_MODE:
                # one text against many images (vilbert.py:780-782): the text rows are broadcast to the image batch
                nb = image_embedding.size(0)
                txt_embedding = txt_embedding.expand(nb, txt_embedding.size(1), txt_embedding.size(2)).contiguous()
                txt_attention_mask = txt_attention_mask.reshape(txt_attention_mask.shape[0], -1).expand(nb, txt_embedding.size(1)).contiguous().view(
                    nb, 1, 1, txt_embedding.size(1))
            if self.with_coattention and recompute_layers:
                c_layer, use_co = self.c_layer[count], bool(self.use_co_attention_mask)
                co_grad = torch.is_tensor(co_attention_mask) and co_attention_mask.requires_grad          # a trainable co_attention_mask
                image_embedding, txt_embedding = _recompute_layer(
                    lambda hv, ht, co, mv, mt, layer=c_layer, use_co=use_co, plans=_Runtime.plans:
                        _with_plans(plans, layer, hv, mv, ht, mt, co, use_co)[:2],
                    (image_embedding, txt_embedding) + ((co_attention_mask,) if co_grad else ()),
                    (() if co_grad else (co_attention_mask,)) + (image_attention_mask, txt_attention_mask))
            elif self.with_coattention:
                image_embedding, txt_embedding, co_probs = self.c_layer[count](
                    image_embedding, image_attention_mask, txt_embedding, txt_attention_mask, co_attention_mask,
                    bool(self.use_co_attention_mask))
                if output_all_attention_masks:
                    att_c.append(co_probs)
                if cuts:
                    image_embedding, txt_embedding = self._cut(f"c{count}", image_embedding, txt_embedding)
            v_start, t_start = v_end, t_end
            if output_all_encoded_layers:
                all_t.append(txt_embedding)
                all_v.append(image_embedding)
        with _live(1):
            image_embedding = run(self.v_layer, v_start, len(self.v_layer), image_embedding, image_attention_mask, att_v, 0, "v")
        with ts.side(txt_embedding, txt_attention_mask), _live(0):
            txt_embedding = run(self.layer, t_start, len(self.layer), txt_embedding, txt_attention_mask, att_t, 0, "t")
        ts.end(txt_embedding, *all_t, *(p for p in att_t if p is not None))
        if not output_all_encoded_layers:
            all_t.append(txt_embedding)
            all_v.append(image_embedding)
        return all_t, all_v, (att_t, att_v, att_c)


class _PoolerBase(nn.Module):
    def _build(self, hidden, bi_hidden):
        self.dense = nn.Linear(hidden, bi_hidden)
        self.activation = nn.ReLU()

    def forward(self, hidden_states):
        # first token of every row, read in place through the GEMM's leading dimension (no gather copy)
        return ops.linear(hidden_states[:, 0], self.dense.weight, self.dense.bias, "relu", out_fp32=True)      # (fp32 out: only matters on the bf16-resident path)


class BertTextPooler(_PoolerBase):
    def __init__(self, config):
        super().__init__()
        self._build(config.hidden_size, config.bi_hidden_size)


class BertImagePooler(_PoolerBase):
    def __init__(self, config):
        super().__init__()
        self._build(config.v_hidden_size, config.bi_hidden_size)


class _HeadTransformBase(nn.Module):
    def _build(self, hidden, act):
        self.dense = nn.Linear(hidden, hidden)
        self.transform_act_fn = act
        self.LayerNorm = BertLayerNorm(hidden, eps=1e-12)

    def forward(self, hidden_states):
        h = ops.linear(hidden_states, self.dense.weight, self.dense.bias, _act_name(self.transform_act_fn))
        return self.LayerNorm(h)


class BertPredictionHeadTransform(_HeadTransformBase):
    def __init__(self, config):
        super().__init__()
        self._build(config.hidden_size, config.hidden_act)


class BertImgPredictionHeadTransform(_HeadTransformBase):
    def __init__(self, config):
        super().__init__()
        # the reference tests config.hidden_act and then applies ACT2FN[config.hidden_act] (vilbert.py:874-879)
        self._build(config.v_hidden_size, config.hidden_act if isinstance(config.hidden_act, str) else config.v_hidden_act)


class BertLMPredictionHead(nn.Module):
    def __init__(self, config, bert_model_embedding_weights):
        super().__init__()
        self.transform = BertPredictionHeadTransform(config)
        self.decoder = nn.Linear(bert_model_embedding_weights.size(1), bert_model_embedding_weights.size(0), bias=False)
        self.decoder.weight = bert_model_embedding_weights          # tied to the word embedding (vilbert.py:901)
        self.bias = nn.Parameter(torch.zeros(bert_model_embedding_weights.size(0)))

    def forward(self, hidden_states):
        return ops.linear(self.transform(hidden_states), self.decoder.weight, self.bias)       # bf16 logits on the bf16-resident path (the loss kernels read them)


class BertOnlyMLMHead(nn.Module):
    def __init__(self, config, bert_model_embedding_weights):
        super().__init__()
        self.predictions = BertLMPredictionHead(config, bert_model_embedding_weights)

    def forward(self, sequence_output):
        return self.predictions(sequence_output)


class BertOnlyNSPHead(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.seq_relationship = nn.Linear(config.hidden_size, 2)

    def forward(self, pooled_output):
        return ops.linear(pooled_output, self.seq_relationship.weight, self.seq_relationship.bias)


class BertImagePredictionHead(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.transform = BertImgPredictionHeadTransform(config)
        self.decoder = nn.Linear(config.v_hidden_size, config.v_target_size)

    def forward(self, hidden_states):
        return ops.linear(self.transform(hidden_states), self.decoder.weight, self.decoder.bias)


class BertPreTrainingHeads(nn.Module):
    def __init__(self, config, bert_model_embedding_weights):
        super().__init__()
        self.predictions = BertLMPredictionHead(config, bert_model_embedding_weights)
        self.bi_seq_relationship = nn.Linear(config.bi_hidden_size, 2)
        self.imagePredictions = BertImagePredictionHead(config)
        self.fusion_method = config.fusion_method
        self.dropout = nn.Dropout(0.1)

    def forward(self, sequence_output_t, sequence_output_v, pooled_output_t, pooled_output_v, heads=("t", "v", "rel"), rows=None, live=None):
        """Returns (prediction_scores_t, prediction_scores_v, seq_relationship_score) like vilbert.py:939-954.
        `heads` lets a caller that discards a head (Lily, lily.py:87) skip its GEMMs; skipped entries are None.
        `rows` = {"t": idx, "v": idx} (optional) decodes only the listed rows of the flattened [N*T, H] / [N*R, Hv] sequences
        (loss-aware heads: the scores come back as [len(idx), vocab] instead of [N, T, vocab]).
        `live` = BertModel.live_rows of the forward that produced the sequences: the transforms' and decoders' weight gradients contract over
        the valid rows (a head that decodes gathered `rows` keeps the plain launch)."""
        live_t = None if live is None or (rows is not None and "t" in rows) else live[0]
        live_v = None if live is None or (rows is not None and "v" in rows) else live[1]
        if rows is not None:
            if "t" in rows:
                sequence_output_t = ops.gather_rows(sequence_output_t.reshape(-1, sequence_output_t.shape[-1]), rows["t"])
            if "v" in rows:
                sequence_output_v = ops.gather_rows(sequence_output_v.reshape(-1, sequence_output_v.shape[-1]), rows["v"])
        if self.fusion_method == "sum":
            pooled = pooled_output_t + pooled_output_v
        elif self.fusion_method == "mul":
            pooled = pooled_output_t * pooled_output_v
        else:
            assert False
        with ops.live_rows_scope(live_t):
            scores_t = self.predictions(sequence_output_t) if "t" in heads else None
        rel = None
        if "rel" in heads:
            pooled = ops.dropout(pooled, self.dropout.p, self.training, _drop_state(self, pooled))
            rel = ops.linear(pooled, self.bi_seq_relationship.weight, self.bi_seq_relationship.bias)
        with ops.live_rows_scope(live_v):
            scores_v = self.imagePredictions(sequence_output_v) if "v" in heads else None
        return scores_t, scores_v, rel


class BertPreTrainedModel(nn.Module):
    """Weight initialisation and checkpoint loading (vilbert.py:972-1179)."""

    def __init__(self, config, default_gpu=True, *inputs, **kwargs):
        super().__init__()
        self.config = config

    def init_bert_weights(self, module):
        if isinstance(module, (nn.Linear, nn.Embedding)):
            module.weight.data.normal_(mean=0.0, std=self.config.initializer_range)
        elif isinstance(module, BertLayerNorm):
            module.bias.data.zero_()
            module.weight.data.fill_(1.0)
        if isinstance(module, nn.Linear) and module.bias is not None:
            module.bias.data.zero_()

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, config, default_gpu=True, state_dict=None, cache_dir=None,
                        from_tf=False, *inputs, **kwargs):
        """Instantiate and load a local PyTorch checkpoint (`.bin`, or a directory holding `pytorch_model.bin`).
        Same key handling as the reference: `model_state_dict` unwrapping (:1104), gamma/beta renames (:1119-1129),
        optional `bert.` prefix (:1155-1159), non-strict with missing / unexpected keys logged (:1161-1172).
        Network download (cached_path) and TensorFlow checkpoints are out of scope."""
        if from_tf:
            raise NotImplementedError("TensorFlow checkpoints are out of scope for the HIP path")
        model = cls(config, *inputs, **kwargs)
        if state_dict is None:
            path = str(pretrained_model_name_or_path)
            if os.path.isdir(path):
                path = os.path.join(path, "pytorch_model.bin")
            if not os.path.exists(path):
                raise RuntimeError(f"checkpoint {path} not found (remote archives are not supported)")
            if default_gpu:
                logger.info("loading archive file {}".format(path))
            state_dict = torch.load(path, map_location="cpu")
            if "model_state_dict" in state_dict:
                state_dict = state_dict["model_state_dict"]
            if "state_dict" in dir(state_dict):
                state_dict = state_dict.state_dict()
        state_dict = {k.replace("gamma", "weight").replace("beta", "bias"): v for k, v in state_dict.items()}
        if not hasattr(model, "bert") and any(s.startswith("bert.") for s in state_dict):
            state_dict = {k[len("bert."):]: v for k, v in state_dict.items() if k.startswith("bert.")}
        result = model.load_state_dict(state_dict, strict=False)
        if result.missing_keys and default_gpu:
            logger.info("Weights of {} not initialized from pretrained model: {}".format(model.__class__.__name__, result.missing_keys))
        if result.unexpected_keys and default_gpu:
            logger.info("Weights from pretrained model not used in {}: {}".format(model.__class__.__name__, result.unexpected_keys))
        return model


def _stays_bf16(x, rows: int, weight) -> bool:
    """Region features that arrive as bf16 (a frame pool's `expand_masked(feature_dtype=torch.bfloat16)`) enter the feature projection as they
    are when that projection, fed `rows` fp32 rows, would have rounded them to bf16 itself (`ops._bf16_eligible`): bf16 -> fp32 -> bf16 is the
    identity, so the outputs are bit for bit those of the converted input, with one cast launch fewer.  Anything else is converted to fp32."""
    return (x.dtype == torch.bfloat16 and x.is_contiguous() and x.data_ptr() % 16 == 0
            and ops._bf16_eligible(rows, weight.shape[0], x.shape[-1]))


class BertImageEmbeddings(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.image_embeddings = nn.Linear(config.v_feature_size, config.v_hidden_size)
        self.image_location_embeddings = nn.Linear(5, config.v_hidden_size)
        self.image_orientation_embeddings = nn.Linear(4, config.v_hidden_size)
        self.image_next_orientation_embeddings = nn.Linear(2, config.v_hidden_size)
        self.image_sequence_embeddings = nn.Embedding(32, config.v_hidden_size)
        self.LayerNorm = BertLayerNorm(config.v_hidden_size, eps=1e-12)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)

    def forward(self, input_ids, input_loc):
        if input_ids.dtype != torch.float32 and not _stays_bf16(input_ids, input_ids.numel() // max(input_ids.shape[-1], 1),
                                                                self.image_embeddings.weight):
            input_ids = input_ids.float()
        if input_loc.dtype != torch.float32:
            input_loc = input_loc.float()
        img = ops.linear(input_ids, self.image_embeddings.weight, self.image_embeddings.bias)
        return ops.image_embed(img, input_loc, self.image_location_embeddings.weight, self.image_location_embeddings.bias,
                               self.image_orientation_embeddings.weight, self.image_orientation_embeddings.bias,
                               self.image_next_orientation_embeddings.weight, self.image_next_orientation_embeddings.bias,
                               self.image_sequence_embeddings.weight, self.LayerNorm.weight, self.LayerNorm.bias,
                               self.LayerNorm.variance_epsilon, _p(self, self.dropout.p), _drop_state(self, img))


class BertModel(BertPreTrainedModel):
    """Two-stream encoder; signature and returns of vilbert.py:1242-1337."""

    def __init__(self, config):
        super().__init__(config)
        self.embeddings = BertEmbeddings(config)
        self.v_embeddings = BertImageEmbeddings(config)
        self.encoder = BertEncoder(config)
        self.t_pooler = BertTextPooler(config)
        self.v_pooler = BertImagePooler(config)
        self.apply(self.init_bert_weights)
        # activation recomputation is an attribute of the encoder; a run that carries its settings in `config.args` (as get_optimization reads
        # args.max_grad_norm) switches it on with args.recompute.  No such field: the attribute keeps its default.
        args = getattr(config, "args", None)
        if args is not None and hasattr(args, "recompute"):
            self.encoder.recompute = args.recompute
        if args is not None and hasattr(args, "skip_padding"):
            self.skip_padding = args.skip_padding
        self.live_rows = None                 # (text LiveRows | None, image LiveRows | None) of the last forward when it built them, for the prediction heads
        self.padding_overflow = None          # device int64 [2] (text, image) once a skip_padding forward has run: valid rows that did not fit, summed

    # Extension, opt-in (a plain attribute like encoder.recompute; taken from config.args.skip_padding when that field exists): padding-free
    # execution.  Both streams run their row-wise kernels -- Linear / FFN GEMMs, LayerNorm, activations, the image embedding -- on the VALID rows
    # of the batch only, packed into [1, capacity, H]; the attention sites move rows to the padded layout and back (ops.rows_unpack / rows_pack),
    # and the last hidden states come back as [N, T, H] / [N, R, H] with exact zeros on padded rows.
    #   None              (default) today's path, bit for bit: no plan, no new launch.
    #   f in (0, 1]       static capacity min(rows, ceil(f * rows / 256) * 256) per side, or a (text, image) pair of fractions.  No host sync,
    #                     capturable.  Valid rows beyond the capacity are DROPPED and counted in `padding_overflow` (train_step reports it).
    #   "exact"           the count of valid rows is read on the host (one sync per side) and rounded up to 256.  Raises under stream capture.
    # A side whose mask argument is None stays padded.  Valid are the rows whose mask entry is non-zero; padded rows are keys behind a -10000
    # additive mask (their softmax weight is exactly 0) and no loss reads them, so losses and gradients are those of the padded run at p = 0.
    # With dropout on, the LayerNorm / FFN / image-embedding sites hash packed coordinates: other masks of the same distribution.
    skip_padding = None

    # Weight gradients over the valid rows only (run-time option GEMM_LIVE_ROWS).  The gradient of every projection's output
    # is exactly zero on a padded row -- padded rows are keys behind the -10000 mask (exp gives exactly 0), the poolers read row 0, LayerNorm /
    # GELU' / dropout backward map a zero row to a zero row -- PROVIDED no loss reads a padded row of the sequence outputs.  That holds for the
    # pre-training losses (ignore_index / target masks), so the pre-training model (Lily) switches it on for its encoder; a bare BertModel and
    # the models that hand per-row outputs to arbitrary losses (VILBertForVLTasks) keep the plain launches.
    wgrad_live_rows = False
    # Run-time option GEMM_LIVE_M: under the same premise the forward and input-gradient GEMMs compute the valid rows only.  Their launch plans
    # want the row count on the HOST, and the count lives on the device: every eager forward posts a copy of it into pinned memory behind an
    # event, and the next forward that finds the event complete uses the value, rounded up to 256 rows (_RowsHint: never a sync, never a wait; a
    # wrong guess costs time, not rows).  `rows_hint` = (text, image) pins the guesses instead (tests, experiments); None = the posted counts.
    rows_hint = None
    _rows_hints = None
    # The INPUT-GRADIENT GEMMs take the list whenever it exists: dY is zero on a padded row, so dX is what it was, bit for bit.  The FORWARD
    # GEMMs take it only when this is set (default off, also for Lily): a listed projection returns zeros on its padded rows, and although
    # no loss reads them they travel row-wise through every later layer into the padded rows of the sequence outputs and of the prediction
    # scores the model returns -- which callers may look at, and the full-model goldens do.
    forward_live_rows = False

    def forward(self, input_txt, input_imgs, image_loc, token_type_ids=None, attention_mask=None, image_attention_mask=None,
                co_attention_mask=None, output_all_encoded_layers=False, output_all_attention_masks=False):
        if not input_imgs.is_cuda:
            raise RuntimeError("ytvln BertModel runs on a HIP device only (inputs are on %s); there is no CPU fallback" % input_imgs.device)
        _begin_forward(self, input_imgs.device)
        n, t = input_txt.shape
        r = input_imgs.size(1)
        # additive masks: 0 where attended, -10000 where padded (vilbert.py:1268-1287); kept as [N,1,1,T] like the reference
        if attention_mask is None:
            ext_t = torch.zeros((n, 1, 1, t), dtype=torch.float32, device=input_txt.device)
        else:
            ext_t = ((1.0 - attention_mask.to(torch.float32)) * -10000.0).view(n, 1, 1, t)
        nv = input_imgs.size(0)          # (differs from the text batch only in fast_mode: one text against many images)
        if image_attention_mask is None:
            ext_v = torch.zeros((nv, 1, 1, r), dtype=torch.float32, device=input_txt.device)
        else:
            ext_v = ((1.0 - image_attention_mask.to(torch.float32)) * -10000.0).view(nv, 1, 1, r)
        # co_attention_mask only feeds the use_co_attention_mask branch, which the reference switches off (vilbert.py:736): materialised
        # (vilbert.py:1289-1298: zeros when None, unsqueeze(1) * 5.0, fp32) only when the encoder's switch is on
        ext_co = None
        if self.encoder.use_co_attention_mask:
            if co_attention_mask is None:
                ext_co = torch.zeros((n, 1, r, t), dtype=torch.float32, device=input_txt.device)
            else:
                ext_co = (co_attention_mask.unsqueeze(1) * 5.0).to(torch.float32)

        ts = ops.TwoStream
        plan_t, plan_v = self._plans(attention_mask, image_attention_mask)          # (None, None) unless skip_padding is set
        self.live_rows = self._live_lists((attention_mask, image_attention_mask), plan_t is not None or plan_v is not None)
        try:
            _Runtime.live = self.live_rows
            if not (self.encoder.in_batch_pairs or self.encoder.FAST_MODE):
                ts.begin(input_imgs.device)              # two-stream mode: the text side starts at its embeddings
                _share_drop_state()
                if ts.active and self.live_rows is not None:          # made on the main stream, read by the text side's backward launches
                    for lr in self.live_rows:
                        if lr is not None:
                            lr.record_stream(ts.side_stream(input_imgs.device))
                if ts.active and plan_t is not None:          # made on the main stream in front of the fork, read by the text side's launches
                    plan_t.record_stream(ts.side_stream(input_imgs.device))
            with ts.side(input_txt, token_type_ids, ext_t):
                embedding_output = self.embeddings(input_txt, token_type_ids)          # padded ids: the kernel derives the position from row % T
                if plan_t is not None:
                    embedding_output = ops.rows_pack(embedding_output, plan_t).view(1, plan_t.capacity, -1)
            if plan_v is not None:          # the 2048-wide feature projection and the fused embedding run on packed rows (bf16 mode: packed, then cast)
                if input_imgs.dtype != torch.float32 and not _stays_bf16(input_imgs, plan_v.capacity, self.v_embeddings.image_embeddings.weight):
                    input_imgs = input_imgs.float()          # (bf16 features the projection would round anyway are packed as bf16 rows)
                input_imgs = ops.rows_pack(input_imgs, plan_v).unsqueeze(0)
                image_loc = ops.rows_pack(image_loc if image_loc.dtype == torch.float32 else image_loc.float(), plan_v).unsqueeze(0)
            with _live(1):
                v_embedding_output = self.v_embeddings(input_imgs, image_loc)
            _Runtime.plans = (plan_t, plan_v) if (plan_t is not None or plan_v is not None) else None
            encoded_layers_t, encoded_layers_v, all_attention_mask = self.encoder(
                embedding_output, v_embedding_output, ext_t, ext_v, ext_co,
                output_all_encoded_layers=output_all_encoded_layers, output_all_attention_masks=output_all_attention_masks)
        finally:
            ts.active = False
            _Runtime.plans = None
            _Runtime.live = None
        if plan_t is not None:          # back to [N, T, H]: padded rows are exact zeros
            encoded_layers_t = [ops.rows_unpack(h.view(plan_t.capacity, -1), plan_t).view(n, t, -1) for h in encoded_layers_t]
        if plan_v is not None:
            encoded_layers_v = [ops.rows_unpack(h.view(plan_v.capacity, -1), plan_v).view(nv, r, -1) for h in encoded_layers_v]
        sequence_output_t, sequence_output_v = encoded_layers_t[-1], encoded_layers_v[-1]
        pooled_output_t = self.t_pooler(sequence_output_t)
        pooled_output_v = self.v_pooler(sequence_output_v)
        if not output_all_encoded_layers:
            encoded_layers_t, encoded_layers_v = encoded_layers_t[-1], encoded_layers_v[-1]
        return encoded_layers_t, encoded_layers_v, pooled_output_t, pooled_output_v, all_attention_mask


    def _plans(self, attention_mask, image_attention_mask):
        """(text RowsPlan | None, image RowsPlan | None) of this forward; accumulates the rows that did not fit into `padding_overflow`."""
        spec = _skip_padding_spec(self.skip_padding)
        if spec is None:
            return None, None
        if self.encoder.in_batch_pairs or self.encoder.FAST_MODE:
            raise NotImplementedError("BertModel.skip_padding with in_batch_pairs / fast_mode: these modes rebuild one stream's rows from the other "
                                      "batch in padded coordinates; run them with skip_padding = None")
        plans = [None if m is None else _side_plan(m, s) for m, s in ((attention_mask, spec[0]), (image_attention_mask, spec[1]))]
        live = [p for p in plans if p is not None]
        if live:
            dev = live[0].counts.device
            if self.padding_overflow is None or self.padding_overflow.device != dev:
                self.padding_overflow = torch.zeros(2, dtype=torch.int64, device=dev)
            zero = self.padding_overflow.new_zeros(())
            self.padding_overflow += torch.stack([zero if p is None else p.counts[1] for p in plans])
        return plans[0], plans[1]

    def _live_lists(self, masks, packed: bool):
        """(text LiveRows | None, image LiveRows | None) of this forward, or None: one list per padding mask, built here and read by the backward
        of every projection of that side (weight gradients over the valid rows only).  Training with gradients on and padded rows only (`packed`
        rows need no list; the pair geometries re-batch one side's rows).  GEMM_LIVE_M: the same lists carry the permutation that lets the
        forward and input-gradient GEMMs of the side leave the padded rows out, and the host's guess of the count for their launch plans
        (_RowsHint)."""
        live_m = ops._lib.option("GEMM_LIVE_M") != 0
        if not (self.wgrad_live_rows and self.training and torch.is_grad_enabled() and not packed and ops.get_matmul_precision() == "fp32"
                and not (self.encoder.in_batch_pairs or self.encoder.FAST_MODE) and (ops._lib.option("GEMM_LIVE_ROWS") != 0 or live_m)):
            return None
        lists = tuple(None if m is None or m.numel() % 32 != 0 else ops.live_rows(m, perm=live_m) for m in masks)
        if live_m:
            if self._rows_hints is None:
                self._rows_hints = (_RowsHint(), _RowsHint())
            for side, lr in enumerate(lists):
                if lr is not None:
                    fixed = None if self.rows_hint is None else self.rows_hint[side]
                    lr.forward = bool(self.forward_live_rows)
                    lr.hint = min(lr.rows, self._rows_hints[side].step(lr.count) if fixed is None else int(fixed))
        return lists if (lists[0] is not None or lists[1] is not None) else None


class BertForMultiModalPreTraining(BertPreTrainedModel):
    """vilbert.py:1373-1455.  Losses run on the fused loss kernels (no host sync)."""

    def __init__(self, config):
        super().__init__(config)
        self.bert = BertModel(config)
        self.cls = BertPreTrainingHeads(config, self.bert.embeddings.word_embeddings.weight)
        self.apply(self.init_bert_weights)
        self.predict_feature = config.predict_feature
        print("model's option for predict_feature is ", config.predict_feature)

    def forward(self, input_ids, image_feat, image_loc, token_type_ids=None, attention_mask=None, image_attention_mask=None,
                masked_lm_labels=None, image_label=None, image_target=None, next_sentence_label=None,
                output_all_attention_masks=False):
        sequence_output_t, sequence_output_v, pooled_output_t, pooled_output_v, all_attention_mask = self.bert(
            input_ids, image_feat, image_loc, token_type_ids, attention_mask, image_attention_mask,
            output_all_encoded_layers=False, output_all_attention_masks=output_all_attention_masks)
        prediction_scores_t, prediction_scores_v, seq_relationship_score = self.cls(
            sequence_output_t, sequence_output_v, pooled_output_t, pooled_output_v, live=self.bert.live_rows)
        if masked_lm_labels is not None and next_sentence_label is not None and image_target is not None:
            n, r, c = prediction_scores_v.shape
            pv = prediction_scores_v[:, 1:].reshape(n * (r - 1), c)                      # region 0 dropped (:1429)
            label = (image_label == 1).reshape(-1)
            if self.predict_feature:
                # MSE feature regression (:1391, 1430-1434): sum((pred - target)^2 over masked regions) / max(#masked * C, 1).  Off in every
                # target config: a handful of elementwise torch kernels on the device, no fused kernel of its own.
                lm = label.to(pv.dtype).unsqueeze(1)
                diff = pv - image_target.reshape(n * (r - 1), c).to(pv.dtype)
                masked_img_loss = (diff * diff * lm).sum() / torch.clamp(lm.sum() * c, min=1.0)
            else:
                # sum(KL * mask) / max(sum(mask), 0): the reference divides by zero when nothing is masked (:1440-1442);
                # the fused kernel clamps the denominator at 1 in that degenerate case.
                masked_img_loss = ops.kl_masked(pv, image_target.reshape(n * (r - 1), c).float(), label)
            masked_lm_loss = ops.cross_entropy(prediction_scores_t.view(-1, self.config.vocab_size), masked_lm_labels.view(-1), -1)
            next_sentence_loss = ops.cross_entropy(seq_relationship_score.view(-1, 2), next_sentence_label.view(-1), -1)
            return masked_lm_loss.unsqueeze(0), masked_img_loss.unsqueeze(0), next_sentence_loss.unsqueeze(0)
        return prediction_scores_t, prediction_scores_v, seq_relationship_score, all_attention_mask


class SimpleClassifier(nn.Module):
    """vilbert.py:1522-1535: Linear -> ReLU -> Dropout -> Linear, both projections weight-normed over the whole matrix (dim=None: `weight_g` is
    0-d).  The two containers are registered through torch's own weight_norm so that construction consumes the reference's generator draws
    and the state-dict keys are `main.{0,3}.{bias,weight_g,weight_v}`; the wrapped Linear is never called -- the effective weight comes from
    ops.weight_norm and feeds the fp32 GEMM in every precision mode (the pooled vectors are fp32, and a weight that is recomputed every
    forward has no bf16 copy in the optimizer's arena to read)."""

    def __init__(self, in_dim, hid_dim, out_dim, dropout):
        super().__init__()
        with warnings.catch_warnings():          # (the hook-based weight_norm is deprecated in torch, and is what names the keys weight_g / weight_v)
            warnings.simplefilter("ignore", FutureWarning)
            first = torch.nn.utils.weight_norm(nn.Linear(in_dim, hid_dim), dim=None)
            last = torch.nn.utils.weight_norm(nn.Linear(hid_dim, out_dim), dim=None)
        self.main = nn.Sequential(first, nn.ReLU(), nn.Dropout(dropout, inplace=True), last)

    def forward(self, x):
        first, drop, last = self.main[0], self.main[2], self.main[3]
        h = ops.LinearFn.apply(x, ops.weight_norm(first.weight_v, first.weight_g), first.bias, "relu")
        h = ops.dropout(h, drop.p, self.training, _drop_state(self, h))
        return ops.LinearFn.apply(h, ops.weight_norm(last.weight_v, last.weight_g), last.bias, None)


class VILBertForVLTasks(BertPreTrainedModel):
    """vilbert.py:1457-1520: the downstream-task model.  Returns (vil_prediction [N, num_labels], vil_logit [N, 1], vil_binary_prediction [N, 2],
    vision_prediction [N, R, v_target], vision_logit [N, R, 1], linguisic_prediction [N, T, vocab], linguisic_logit [N, T, 1]).  The two
    per-row logits run on ops.row_logit (dropout, dot product and region-mask term in one kernel, fp32 out on fp32 or bf16 hidden states)."""

    def __init__(self, config, num_labels, dropout_prob=0.1, default_gpu=True):
        super().__init__(config)
        self.num_labels = num_labels
        self.bert = BertModel(config)
        self.dropout = nn.Dropout(dropout_prob)
        self.cls = BertPreTrainingHeads(config, self.bert.embeddings.word_embeddings.weight)
        self.vil_prediction = SimpleClassifier(config.bi_hidden_size, config.bi_hidden_size * 2, num_labels, 0.5)
        self.vil_logit = nn.Linear(config.bi_hidden_size, 1)
        self.vision_logit = nn.Linear(config.v_hidden_size, 1)
        self.linguisic_logit = nn.Linear(config.hidden_size, 1)
        self.fusion_method = config.fusion_method
        self.apply(self.init_bert_weights)

    def forward(self, input_txt, input_imgs, image_loc, token_type_ids=None, attention_mask=None, image_attention_mask=None,
                co_attention_mask=None, output_all_encoded_layers=False):
        sequence_output_t, sequence_output_v, pooled_output_t, pooled_output_v, _ = self.bert(
            input_txt, input_imgs, image_loc, token_type_ids, attention_mask, image_attention_mask, co_attention_mask,
            output_all_encoded_layers=False)
        linguisic_prediction, vision_prediction, vil_binary_prediction = self.cls(
            sequence_output_t, sequence_output_v, pooled_output_t, pooled_output_v)
        if self.fusion_method == "sum":
            pooled_output = pooled_output_t + pooled_output_v
        elif self.fusion_method == "mul":
            pooled_output = pooled_output_t * pooled_output_v
        else:
            assert False
        p = self.dropout.p
        pooled_output = ops.dropout(pooled_output, p, self.training, _drop_state(self, pooled_output))
        vil_prediction = self.vil_prediction(pooled_output)
        vil_logit = ops.linear(pooled_output, self.vil_logit.weight, self.vil_logit.bias)
        # (the reference has no branch for a missing region mask: it fails on `1.0 - None`; here that means "every region attended")
        vision_logit = ops.row_logit(sequence_output_v, self.vision_logit.weight, self.vision_logit.bias, image_attention_mask, p,
                                     self.training, _drop_state(self, sequence_output_v))
        linguisic_logit = ops.row_logit(sequence_output_t, self.linguisic_logit.weight, self.linguisic_logit.bias, None, p,
                                        self.training, _drop_state(self, sequence_output_t))
        return (vil_prediction, vil_logit, vil_binary_prediction, vision_prediction, vision_logit, linguisic_prediction, linguisic_logit)
