"""CPU: hidden_act = "swish" -- the oracle against the fixtures generated from the reference (tools/gen_golden_swish.py), the C ABI of the
stand-alone activation kernels (header <-> exported symbols <-> ctypes table), and the activation names the model accepts."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import vilbert_ref as O
from conftest import GOLD, ROOT
from helpers import ZERO_DROP, cfg_dict, close, gold, rel_l2
from ytvln import synth

ALL = dict(ranking=True, traj_judge=True, masked_vision=True, masked_language=True)


def micro_weights(g):
    """synth.make_weights(seed 11) on the micro schema; the fixture pins the recipe with one checksum per tensor."""
    shapes = json.load(open(os.path.join(GOLD, "state_dict_schema.json")))["Lily/micro.json"]["shapes"]
    W = synth.make_weights({k: tuple(v) for k, v in shapes.items()}, 11)
    assert list(W) == g["w_names"].tolist()
    for (k, v), s in zip(W.items(), g["w_sum"]):
        assert float(v.astype(np.float64).sum()) == float(s), f"weight recipe drifted for {k}"
    return W


def state(W):
    return {k: torch.from_numpy(v).clone() for k, v in W.items()}


def test_g19_swish_kats_oracle():
    """The bar test_oracle_golden.py holds the oracle's gelu to against g5 (1e-7 / 1e-7), forward and autograd derivative; the fixture covers
    the inputs where a naive sigmoid overflows and is finite everywhere."""
    k = gold("g19_swish_kats.npz")
    x = torch.from_numpy(k["swish/x"]).requires_grad_(True)
    assert np.isfinite(k["swish/y"]).all() and np.isfinite(k["swish/dy"]).all()
    for v in (0.0, 1e-30, 87.0, 89.0, 104.0, 1e4, 3e38):
        assert (k["swish/x"] == np.float32(v)).any() and (k["swish/x"] == np.float32(-v)).any(), v
    assert np.signbit(k["swish/x"][k["swish/x"] == 0]).any()          # -0.0 is there
    y = O._act("swish", x)
    close(y, k["swish/y"], 1e-7, 1e-7, "swish")
    y.sum().backward()
    close(x.grad, k["swish/dy"], 1e-7, 1e-7, "swish'")
    big = k["swish/x"] >= 104
    assert np.array_equal(k["swish/y"][big], k["swish/x"][big]) and (k["swish/dy"][big] == 1).all()
    small = k["swish/x"] <= -104
    assert (k["swish/y"][small] == 0).all() and (k["swish/dy"][small] == 0).all()


def test_g19_swish_micro_oracle():
    """test_g0_micro_forward_losses_grads_and_adamw's bars on the all-swish recipe (logits 2e-5, losses 1e-6, gradient rel-L2 1e-4 with the
    tiny-norm guard, parameters after three AdamW steps 1e-7 / 1e-6), then the mixed case hidden_act = "swish" / v_hidden_act = "gelu".

    Measured: passes on the Intel host the fixture was generated on (1, 8 and 16 threads).  The last bar is the oracle's own fp32 CPU
    arithmetic against the reference's and sits at the edge of what two CPUs agree on: on the AMD host of an MI355X box one element of
    240 of bert.v_embeddings.image_location_embeddings.weight read 1.048e-7 off against a bound of 1.04e-7 (AdamW divides a gradient
    element that is mostly cancellation by its own magnitude).  The bar is g0's and stays."""
    g = gold("g19_swish_micro.npz")
    fl = O.TaskFlags(**ALL)
    W = micro_weights(g)
    nb = synth.make_batch(bs=2, K=3, T=8, frames=2, boxes=3, F=16, C=11, vocab=97, seed=21, opt_holes=1, ignore_rank_frac=0.0)
    for i, a in enumerate(nb):
        assert np.array_equal(a, g["in_%02d" % i]), f"batch recipe drifted at index {i}"
    batch = [torch.from_numpy(g["in_%02d" % i]) for i in range(16)]
    ids, feat, loc, seg, imask, vmask = O.model_input(batch)
    for prefix, v_act in (("", "swish"), ("mixed/", "gelu")):
        cfg = O.RefConfig(**cfg_dict("micro.json", hidden_act="swish", v_hidden_act=v_act, **ZERO_DROP))
        with torch.no_grad():
            out = O.lily_forward(state(W), cfg, fl, ids, feat, loc, seg, imask, vmask)
            total, per = O.total_loss(batch, out, fl)
        for k in ("ranking", "traj", "vision", "language"):
            close(out[k], g[prefix + "logits/" + k], 2e-5, 2e-5, prefix + k)
            close(per[k], g[prefix + "loss/" + k], 1e-6, 1e-6, prefix + k)
        close(total, g[prefix + "loss/total"], 1e-6, 1e-6)
        S, st = state(W), O.AdamWState()
        warm, tot = O.schedule_totals(10, 1, 1)
        for step in range(3 if not prefix else 1):
            lr = 1e-3 * O.warmup_linear(step, warm, tot)
            loss, _, grads, _ = O.train_step(S, cfg, fl, batch, st, lr)
            if not prefix:
                assert abs(lr - float(g[f"step{step}.lr"])) < 1e-12
                close(loss, g[f"step{step}.loss"], 1e-6, 1e-6)
            if step == 0:
                assert {n for n, v in grads.items() if v is None} == set(g["unused"].tolist())
                for n, v in grads.items():
                    if v is not None:
                        ref = g[prefix + "grad/" + n]
                        assert rel_l2(v, ref) < 1e-4 or float(np.linalg.norm(ref)) < 1e-7, (prefix, n)
        if not prefix:
            for n in S:
                if ("after3/" + n) in g.files:
                    close(S[n], g["after3/" + n], 1e-7, 1e-6, n)
    # the two cases differ where, and only where, they should: the text stream and both prediction heads are swish in both
    assert not np.array_equal(g["logits/vision"], g["mixed/logits/vision"])


def test_g19_swish_tiny_oracle():
    """The tiny-config swish fixture (the one the bf16-resident path can run) at the bars test_oracle_golden.py holds g1 / g2 to: losses
    2e-6, logits 5e-5, gradient norms 2e-4, parameter norms after the AdamW step 2e-6."""
    g = gold("g19_swish_tiny.npz")
    cfg = O.RefConfig(**cfg_dict("tiny_2_2_1.json", hidden_act="swish", v_hidden_act="swish", **ZERO_DROP))
    shapes = json.load(open(os.path.join(GOLD, "state_dict_schema.json")))["Lily/tiny_2_2_1.json"]["shapes"]
    S = state(synth.make_weights({k: tuple(v) for k, v in shapes.items()}, 12))
    batch = synth.to_torch(synth.make_batch(bs=2, K=7, T=16, frames=2, boxes=4, seed=22, ignore_rank_frac=0.0))
    loss, per, grads, out = O.train_step(S, cfg, O.TaskFlags(**ALL), batch, O.AdamWState(), float(g["lr"]))
    close(loss, g["loss/total"], 2e-6, 2e-6)
    for k, v in per.items():
        close(v, g["loss/" + k], 2e-6, 2e-6, k)
    for k, v in out.items():
        ref, flat = g["logits/" + k], v.detach().reshape(v.shape[0], -1)
        got = v.detach() if ref.shape == tuple(v.shape) else flat[:, ::int(g["logits_stride/" + k])][:, :ref.shape[1]]
        close(got, ref, 5e-5, 5e-5, k)
    for n, ref in zip(g["grad_names"].tolist(), g["grad_norms"]):
        assert abs(float(grads[n].double().norm()) - ref) <= 2e-4 * ref + 1e-7, n
    assert {n for n, v in grads.items() if v is None} == set(g["unused"].tolist())
    for n, n_ref in zip(g["param_names"].tolist(), g["post_norm"]):
        assert abs(float(S[n].double().norm()) - n_ref) <= 2e-6 * n_ref + 1e-7, n


def _header():
    text = open(os.path.join(ROOT, "include", "ytvln.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_act_fwd_is_declared_exported_and_bound():
    """Header, export table and ctypes table all carry ytvln_act_fwd_f32 / ytvln_act_fwd_bf16 with one signature, and the activation value
    has the same number in the header and in the binding -- above every GEMM epilogue value, which the GEMM entry points reject."""
    import ctypes
    from ytvln import _build, _lib
    _build.build(verbose=False)
    text = _header()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in exported.splitlines() if " T " in l}
    for name, elem in (("ytvln_act_fwd_f32", "float"), ("ytvln_act_fwd_bf16", "uint16_t")):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, f"{name} is not declared in ytvln.h"
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert args == [f"const {elem}* z", f"{elem}* y", "int64_t n", "int act", "void* stream"], args
        assert name in exported, f"{name} is not exported"
        assert _lib.SIGNATURES[name] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    m = re.search(r"\bYTVLN_ACT_SWISH\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == _lib.ACT_SWISH
    epi = {n: int(v) for n, v in re.findall(r"\b(YTVLN_EPI_\w+)\s*=\s*(\d+)", text)}
    assert _lib.ACT_SWISH > max(epi.values()) == epi["YTVLN_EPI_MUL_DRELU"] == _lib.EPI_MUL_DRELU
    assert re.search(r"#define\s+YTVLN_ABI_VERSION\s+2\b", text) and _lib.ABI_VERSION == 2
    # host-side argument checks (no GPU work): only the new value is an activation of these kernels; n = 0 is a no-op; the GEMM refuses it
    lib = _lib.load()
    assert lib.ytvln_act_fwd_f32(16, 16, 0, _lib.ACT_SWISH, None) == 0 and lib.ytvln_act_fwd_bf16(16, 16, 0, _lib.ACT_SWISH, None) == 0
    for act in (_lib.EPI_NONE, _lib.EPI_GELU, _lib.EPI_RELU, 6):
        assert lib.ytvln_act_fwd_f32(16, 16, 0, act, None) != 0 and b"act_fwd" in lib.ytvln_last_error()
        assert lib.ytvln_act_fwd_bf16(16, 16, 0, act, None) != 0
    assert lib.ytvln_act_fwd_f32(None, None, 0, _lib.ACT_SWISH, None) == 0          # an empty tensor has no address
    assert lib.ytvln_act_fwd_f32(None, 16, 4, _lib.ACT_SWISH, None) != 0 and lib.ytvln_act_fwd_f32(16, 16, -1, _lib.ACT_SWISH, None) != 0
    assert lib.ytvln_act_bwd_f32(16, 16, 16, 0, _lib.ACT_SWISH, None) == 0 and lib.ytvln_act_bwd_bf16(16, 16, 16, 0, _lib.ACT_SWISH, None) == 0
    assert lib.ytvln_act_bwd_f32(16, 16, 16, 0, 6, None) != 0
    # (empty problems: even an accepted call would launch nothing)
    rc = lib.ytvln_gemm_f32(16, 4, 0, 16, 4, 1, 16, 4, None, None, 0, 0, 0, 0, _lib.ACT_SWISH, 0.0, None, 0, 0, None)
    assert rc != 0 and b"bad epilogue" in lib.ytvln_last_error()
    with pytest.raises(RuntimeError, match="bad epilogue"):
        _lib.call("ytvln_gemm_bf16", 16, 8, 0, 16, 8, 1, 16, 8, _lib.DT_BF16, None, None, 0, 0, 0, 0, _lib.ACT_SWISH, 0.0, None, 0, 0, None, None, None)


def test_act_name_accepts_the_three_reference_activations_only():
    from ytvln import ops, vilbert
    assert vilbert._act_name("swish") == "swish"
    assert [vilbert._act_name(a) for a in ("gelu", "relu")] == ["gelu", "relu"]
    assert set(vilbert.ACT2FN) == {"gelu", "relu", "swish"} <= set(ops._ACT)
    for bad in ("tanh", vilbert.swish, vilbert.ACT2FN["gelu"], None):
        with pytest.raises(NotImplementedError, match="'gelu'.*'relu'.*'swish'"):
            vilbert._act_name(bad)
    # a swish config constructs every module that applies an activation, and each of them resolves to the HIP path's name
    cfg = vilbert.BertConfig(**cfg_dict("micro.json", hidden_act="swish", v_hidden_act="gelu", **ZERO_DROP))
    assert vilbert._act_name(vilbert.BertIntermediate(cfg).intermediate_act_fn) == "swish"
    assert vilbert._act_name(vilbert.BertImageIntermediate(cfg).intermediate_act_fn) == "gelu"
    assert vilbert._act_name(vilbert.BertPredictionHeadTransform(cfg).transform_act_fn) == "swish"
    assert vilbert._act_name(vilbert.BertImgPredictionHeadTransform(cfg).transform_act_fn) == "swish"      # hidden_act, as in the reference
