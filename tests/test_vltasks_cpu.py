"""CPU: VILBertForVLTasks / SimpleClassifier exist, carry the reference's keys and seeded construction (fixtures from
tools/gen_golden_vltasks.py), the fp64 restatement the GPU tests lean on reproduces the reference's outputs, and the new entry points are
declared, bound and validate their arguments."""
import ctypes
import os
import re
import warnings

import numpy as np
import torch

from conftest import ROOT
from helpers import cfg_dict, gold
from vltasks_common import G_OVERRIDE, MICRO_BATCH, NEW_KEYS, NUM_LABELS, OUT_NAMES, build_model, inputs_of, make_weights, state_of, vltasks_forward

NEW_ENTRY_POINTS = ["ytvln_weight_norm_workspace_elems", "ytvln_weight_norm_fwd_f32", "ytvln_weight_norm_bwd_f32", "ytvln_row_logit_workspace_elems",
                    "ytvln_row_logit_fwd_f32", "ytvln_row_logit_fwd_bf16", "ytvln_row_logit_bwd_f32", "ytvln_row_logit_bwd_bf16"]


def test_the_two_names_exist():
    from ytvln import ops
    from ytvln.vilbert import BertPreTrainedModel, SimpleClassifier, VILBertForVLTasks
    assert issubclass(VILBertForVLTasks, BertPreTrainedModel) and issubclass(SimpleClassifier, torch.nn.Module)
    assert callable(ops.weight_norm) and callable(ops.row_logit)


def test_key_set_and_shapes_equal_the_reference():
    g = gold("g21_vltasks_init.npz")
    from ytvln.vilbert import BertConfig, VILBertForVLTasks
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", FutureWarning)
        sd = VILBertForVLTasks(BertConfig(**cfg_dict("micro.json")), NUM_LABELS).state_dict()
    assert list(sd) == g["names"].tolist()
    assert [",".join(map(str, v.shape)) for v in sd.values()] == g["shapes"].tolist()
    extra = [k for k in sd if not k.startswith(("bert.", "cls."))]
    assert extra == NEW_KEYS
    assert sd["vil_prediction.main.0.weight_g"].shape == () and sd["vil_prediction.main.3.weight_g"].shape == ()


def test_seeded_construction_draws_the_reference_numbers():
    """torch.manual_seed(1234): every tensor's float64 sum and sum of squares (numpy, of the fp32 values) equals the reference's exactly --
    the generator is consumed in the reference's order, the draw into the hook-managed `weight` of the weight-normed Linears included."""
    g = gold("g21_vltasks_init.npz")
    from ytvln.vilbert import BertConfig, VILBertForVLTasks
    torch.manual_seed(1234)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", FutureWarning)
        model = VILBertForVLTasks(BertConfig(**cfg_dict("micro.json")), NUM_LABELS)
    for k, v, s, ss in zip(model.state_dict(), model.state_dict().values(), g["sum"], g["sumsq"]):
        a = v.detach().numpy().astype(np.float64)
        assert float(np.sum(a)) == float(s) and float(np.sum(a * a)) == float(ss), k
    sd = model.state_dict()
    for pre, fan_in in (("vil_prediction.main.0", 32), ("vil_prediction.main.3", 64)):
        v = sd[pre + ".weight_v"]
        assert float(v.abs().max()) <= 1.0 / np.sqrt(fan_in)                      # nn.Linear's default init, not N(0, 0.02)
        assert abs(float(sd[pre + ".weight_g"]) - float(v.norm())) < 1e-6 and float(sd[pre + ".bias"].abs().max()) == 0.0


def test_restatement_reproduces_the_reference_outputs():
    """|delta| <= 1e-5 + 1e-5 |ref| on all 7 outputs, both fusion methods; the recipes (weights, batch, mask) rebuild the fixture's inputs."""
    import vilbert_ref as O
    from helpers import ZERO_DROP
    from ytvln import synth
    g = gold("g21_vltasks_micro.npz")
    assert dict(zip(g["g_names"].tolist(), g["g_values"].tolist())) == G_OVERRIDE
    nb = synth.make_batch(**MICRO_BATCH)
    for i, a in enumerate(nb):
        assert np.array_equal(a, g["in_%02d" % i]), f"batch recipe drifted at index {i}"
    mask = g["region_mask"]
    assert mask[0].all() and not mask[1, -2:].any() and mask[1, :-2].all() and not mask[2, -4:].any() and mask[2, :-4].all()
    inp = inputs_of(nb, mask)
    W = make_weights(build_model("micro.json"), 41)
    for fusion, pre in (("mul", ""), ("sum", "sum/")):
        cfg = O.RefConfig(**cfg_dict("micro.json", fusion_method=fusion, **ZERO_DROP))
        with torch.no_grad():
            outs = vltasks_forward(state_of(W, torch.float64), cfg, *inp)
        for n, o in zip(OUT_NAMES, outs):
            ref = torch.from_numpy(g[pre + "out/" + n]).double()
            assert o.shape == ref.shape, n
            err = (o - ref).abs()
            assert bool((err <= 1e-5 + 1e-5 * ref.abs()).all()), f"{pre}{n}: max abs err {float(err.max()):.3e}"
    assert [tuple(g["out/" + n].shape) for n in OUT_NAMES] == [(3, 7), (3, 1), (3, 2), (3, 10, 11), (3, 10, 1), (3, 12, 97), (3, 12, 1)]


def test_new_entry_points_are_declared_bound_and_validate():
    from ytvln import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ytvln.h")).read(), flags=re.S)
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b(int64_t|int)\s+%s\s*\(" % name, text), f"{name} not declared in ytvln.h"
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 2
    try:
        lib = _lib.load()
    except _lib.YtvlnLibraryError:
        return          # not built here: the header / table half above is all a CPU run can say
    assert lib.ytvln_weight_norm_workspace_elems(4) == 1 and lib.ytvln_weight_norm_workspace_elems(64 * 32 + 4) == 3
    assert lib.ytvln_weight_norm_workspace_elems(1024 * 2048) == 256
    assert lib.ytvln_row_logit_workspace_elems(1, 48) == 52 and lib.ytvln_row_logit_workspace_elems(1000, 256) == 63 * 260
    assert lib.ytvln_row_logit_workspace_elems(16128, 1024) == 1008 * 1028 and lib.ytvln_row_logit_workspace_elems(129024, 1024) == 1024 * 1028
    P = ctypes.c_void_p
    for fn, h_bad in ((lib.ytvln_row_logit_fwd_f32, 30), (lib.ytvln_row_logit_fwd_bf16, 36)):
        rc = fn(P(16), 64, P(16), None, None, P(16), 4, h_bad, 0.0, None, 0, None)                 # H off the vector granule
        assert rc < 0 and b"row_logit_fwd" in lib.ytvln_last_error() and b"H=" in lib.ytvln_last_error()
        rc = fn(P(16), 64, P(16), None, None, P(16), 4, 64, 1.0, P(16), 0, None)                   # p = 1
        assert rc < 0 and b"p out of range" in lib.ytvln_last_error()
        assert fn(P(16), 64, P(16), None, None, P(16), 4, 64, 0.5, None, 0, None) < 0 and b"rng" in lib.ytvln_last_error()
        assert fn(P(16), 64, P(16), None, None, P(16), 4, 4096, 0.0, None, 0, None) < 0            # H > 2048
        assert fn(P(16), 60, P(16), None, None, P(16), 4, 64, 0.0, None, 0, None) < 0              # ldx < H
        assert fn(P(24), 64, P(16), None, None, P(16), 4, 64, 0.0, None, 0, None) < 0 and b"aligned" in lib.ytvln_last_error()
    for fn in (lib.ytvln_row_logit_bwd_f32, lib.ytvln_row_logit_bwd_bf16):
        rc = fn(P(16), 64, P(16), P(16), 4, 30, 0.0, None, 0, P(16), 64, P(16), None, P(16), None)
        assert rc < 0 and b"row_logit_bwd" in lib.ytvln_last_error()
        assert fn(P(16), 64, P(16), P(16), 4, 64, 1.0, P(16), 0, P(16), 64, P(16), None, P(16), None) < 0
    assert lib.ytvln_weight_norm_fwd_f32(None, None, 4, None, None, None, None, None) < 0 and b"weight_norm_fwd" in lib.ytvln_last_error()
    assert lib.ytvln_weight_norm_fwd_f32(P(16), P(16), 0, P(16), None, P(16), P(16), None) < 0
    assert lib.ytvln_weight_norm_bwd_f32(P(20), P(16), P(16), 4, P(16), P(16), P(16), None) < 0 and b"aligned" in lib.ytvln_last_error()
