"""CPU: the ABI of the per-score attention bias (header <-> ctypes table <-> record sizes) and the stride helper that maps the accepted bias
shapes -- and the transposed view the co-attention mask is read through -- to (stride_n, stride_h, stride_q, stride_k)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

NEW = ("ytvln_attn_bias_size", "ytvln_attn_fwd_bias_f32", "ytvln_attn_bwd_bias_f32", "ytvln_attn_fwd_bias_bf16", "ytvln_attn_bwd_bias_bf16",
       "ytvln_attn_probs_bias_f32")


def test_header_declares_the_bias_record_and_entry_points_and_the_binding_matches():
    import __graft_entry__ as g
    g.build()
    from ytvln import _lib
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "ytvln.h")).read()
    body = re.search(r"typedef struct ytvln_attn_bias \{(.*?)\} ytvln_attn_bias;", text, flags=re.S)
    assert body, "ytvln_attn_bias is not declared"
    fields = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    assert re.search(r"const float\s*\*\s*ptr;", fields)
    assert re.search(r"int64_t stride_n, stride_h, stride_q, stride_k;", fields)
    assert [n for n, _ in _lib.AttnBias._fields_] == ["ptr", "stride_n", "stride_h", "stride_q", "stride_k"]
    assert lib.ytvln_attn_bias_size() == ctypes.sizeof(_lib.AttnBias) == 40
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    pair = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 3 + [ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
    for name in NEW[1:5]:
        assert _lib.SIGNATURES[name] == pair, name
    # the old contract is intact: ABI version 2, the 192-byte problem record
    assert lib.ytvln_version() == _lib.ABI_VERSION == 2
    assert re.search(r"#define YTVLN_ABI_VERSION 2\b", text)
    assert lib.ytvln_attn_problem_size() == ctypes.sizeof(_lib.AttnProblem) == 192


def test_bias_entry_points_validate_their_arguments_without_a_gpu():
    from ytvln import _lib
    lib = _lib.load()
    pr = _lib.AttnProblem()
    assert lib.ytvln_attn_fwd_bias_f32(None, None, None, None, 1, 1, 64, 0.125, None, None) != 0 and b"null problem" in lib.ytvln_last_error()
    assert lib.ytvln_attn_bwd_bias_bf16(ctypes.addressof(pr), None, None, None, 0, 1, 64, 0.125, None, None) != 0
    assert b"positive" in lib.ytvln_last_error()
    pr.Tq, pr.Tk = 4, 4
    b = _lib.AttnBias()
    b.ptr, b.stride_q, b.stride_k = 6, 4, 1          # not 4-byte aligned
    assert lib.ytvln_attn_fwd_bias_f32(ctypes.addressof(pr), ctypes.addressof(b), None, None, 1, 1, 64, 0.125, None, None) != 0
    assert b"4-byte aligned" in lib.ytvln_last_error()
    b.ptr, b.stride_q = 8, -4
    assert lib.ytvln_attn_fwd_bias_bf16(ctypes.addressof(pr), ctypes.addressof(b), None, None, 1, 1, 64, 0.125, None, None) != 0
    assert b"non-negative" in lib.ytvln_last_error()
    b.stride_q = 1 << 31
    assert lib.ytvln_attn_probs_bias_f32(8, 64, 8, 64, None, ctypes.addressof(b), 8, 8, 1, 1, 4, 4, 64, 0.125, None) != 0
    assert b"2^31" in lib.ytvln_last_error()


def test_stride_helper_maps_the_accepted_shapes_and_the_transposed_view():
    from ytvln import ops
    N, h, Tq, Tk = 3, 4, 5, 7
    f = ops.attn_bias_strides
    assert f(torch.zeros(N, 1, Tq, Tk), N, h, Tq, Tk) == (Tq * Tk, 0, Tk, 1)
    assert f(torch.zeros(N, h, Tq, Tk), N, h, Tq, Tk) == (h * Tq * Tk, Tq * Tk, Tk, 1)
    assert f(torch.zeros(1, 1, Tq, Tk), N, h, Tq, Tk) == (0, 0, Tk, 1)
    co = torch.zeros(N, 1, Tk, Tq)                       # [N,1,R,T] read by the tokens-over-regions direction: swapped strides, same storage
    v = co.transpose(2, 3)
    assert v.data_ptr() == co.data_ptr() and f(v, N, h, Tq, Tk) == (Tq * Tk, 0, 1, Tq)
    assert f(torch.zeros(1, 1, Tq, Tk).expand(N, h, Tq, Tk), N, h, Tq, Tk) == (0, 0, Tk, 1)      # an expanded view broadcasts by stride 0
    assert f(torch.zeros(N, 1, Tq, 2 * Tk)[..., ::2], N, h, Tq, Tk) == (2 * Tq * Tk, 0, 2 * Tk, 2)   # any positive strides, as it lies
    for bad in (torch.zeros(N, Tq, Tk), torch.zeros(N, 1, Tq, Tk + 1), torch.zeros(2, 1, Tq, Tk), torch.zeros(N, 2, Tq, Tk)):
        with pytest.raises(NotImplementedError, match="accepted are"):
            f(bad, N, h, Tq, Tk)
    with pytest.raises(RuntimeError, match="requires_grad"):
        ops._attn_bias(torch.zeros(N, 1, Tq, Tk, requires_grad=True), N, h, Tq, Tk)
    with pytest.raises(RuntimeError, match="GPU"):
        ops._attn_bias(torch.zeros(N, 1, Tq, Tk), N, h, Tq, Tk)


def test_self_attention_mask_routing():
    """N*T elements: the per-key path; [N,1,T,T], [N,h,T,T], [1,1,T,T]: the bias operand with no key mask; anything else is refused."""
    from ytvln.vilbert import _self_mask
    N, h, T = 3, 4, 6
    m, b = _self_mask(torch.zeros(N, 1, 1, T), N, T, h)
    assert tuple(m.shape) == (N, T) and b is None
    for shape in ((N, 1, T, T), (N, h, T, T), (1, 1, T, T)):
        x = torch.zeros(shape)
        m, b = _self_mask(x, N, T, h)
        assert m is None and b is x
    for shape in ((N, T, T), (N, 1, T, T + 1), (2, 1, T, T), (1, h, T, T)):
        with pytest.raises(NotImplementedError, match="accepted are"):
            _self_mask(torch.zeros(shape), N, T, h)


def test_encoder_switch_is_a_plain_attribute_not_a_config_field():
    import dataclasses
    from ytvln.vilbert import BertConfig, BertEncoder
    assert BertEncoder.use_co_attention_mask is False
    assert "use_co_attention_mask" not in {f.name for f in dataclasses.fields(BertConfig)}


# ---- the g20 fixtures (from the real reference) agree with an fp64 restatement written here, and are small -------------------------------
def _mha(q, k, v, mask, bias, heads):
    N, Tq, H = q.shape
    d = H // heads
    qh, kh, vh = (t.view(N, -1, heads, d).permute(0, 2, 1, 3) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) / d ** 0.5 + mask + bias
    pr = torch.softmax(s, -1)
    return (pr @ vh).permute(0, 2, 1, 3).reshape(N, Tq, H), pr


def _weights(shapes, seed):
    import numpy as np
    from ytvln import synth
    W = synth.make_weights(shapes, seed)
    return {k: torch.from_numpy((v * 10.0).astype(np.float32) if k.endswith("weight") and ("query" in k or "key" in k) else v).double()
            for k, v in W.items()}


def test_g20_fixture_files_are_small():
    from conftest import GOLD
    files = [f for f in os.listdir(GOLD) if f.startswith("g20_attn_bias_")]
    assert len(files) == 5, files
    for f in files:
        assert os.path.getsize(os.path.join(GOLD, f)) < (1 << 20), f


def test_g20_self_attention_fixture_agrees_with_fp64():
    from helpers import close, gold
    g = gold("g20_attn_bias_self.npz")
    for tag, heads in (("t", 4), ("v", 4)):
        names = list(g[f"{tag}/w_names"])
        x = torch.from_numpy(g[f"{tag}/x"]).double()
        W = _weights({n: ((x.shape[-1], x.shape[-1]) if n.endswith("weight") else (x.shape[-1],)) for n in names}, int(g[f"{tag}/seed"]))
        q, k, v = (x @ W[f"{n}.weight"].t() + W[f"{n}.bias"] for n in ("query", "key", "value"))
        for mname in ("causal", "block", "heads"):
            ctx, pr = _mha(q, k, v, 0.0, torch.from_numpy(g[f"{tag}/{mname}/mask"]).double(), heads)
            close(g[f"{tag}/{mname}/ctx"], ctx, 2e-6, 2e-5, f"{tag}/{mname} context")
            close(g[f"{tag}/{mname}/probs"], pr, 2e-6, 2e-5, f"{tag}/{mname} probabilities")


def test_g20_connection_fixture_probabilities_agree_with_fp64():
    """Which direction reads the mask transposed (vilbert.py:581-582 against :603-604) is what a wrong fixture -- or a wrong reading of the
    reference -- would get wrong: probs1 [N,h,T,R] uses co^T, probs2 [N,h,R,T] uses co."""
    import json
    from conftest import CFG_DIR
    from helpers import close, gold
    g = gold("g20_attn_bias_conn_micro.npz")
    cfg = json.load(open(os.path.join(CFG_DIR, "micro.json")))
    names = list(g["w_names"])
    hb, hv, ht = cfg["bi_hidden_size"], cfg["v_hidden_size"], cfg["hidden_size"]
    shapes = {}
    from ytvln.vilbert import BertConfig, BertConnectionLayer
    layer = BertConnectionLayer(BertConfig(**cfg))
    shapes = {k: tuple(v.shape) for k, v in layer.state_dict().items()}
    assert sorted(shapes) == sorted(names)
    W = _weights(shapes, int(g["seed"]))
    x1, x2 = torch.from_numpy(g["x1"]).double(), torch.from_numpy(g["x2"]).double()
    lin = lambda x, n: x @ W[f"biattention.{n}.weight"].t() + W[f"biattention.{n}.bias"]          # noqa: E731
    co = torch.from_numpy(g["co"]).double()
    _, p1 = _mha(lin(x2, "query2"), lin(x1, "key1"), lin(x1, "value1"), torch.from_numpy(g["m1"]).double(), co.permute(0, 1, 3, 2), 4)
    _, p2 = _mha(lin(x1, "query1"), lin(x2, "key2"), lin(x2, "value2"), torch.from_numpy(g["m2"]).double(), co, 4)
    close(g["probs1"], p1, 2e-6, 2e-5, "probs1")
    close(g["probs2"], p2, 2e-6, 2e-5, "probs2")
    assert hb and hv and ht


def test_g20_model_fixture_moves_the_logits():
    import numpy as np
    from helpers import gold
    g, g0 = gold("g20_attn_bias_model.npz"), gold("g0_micro.npz")
    assert set(np.unique(g["co"])) <= {-1.0, 0.0, 1.0}
    assert max(float(np.abs(g["logits/" + k] - g0["logits/" + k]).max()) for k in ("vision", "language")) > 2e-3
