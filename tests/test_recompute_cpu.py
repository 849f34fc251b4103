"""CPU: activation recomputation (BertEncoder.recompute) -- the C ABI of the GELU recomputation kernel (header <-> exported symbols <-> ctypes
table, host-side argument checks), the dropout replay helper on a stand-in state object, the attribute rule of BertModel, and the guards that
need no device (they raise before the first launch)."""
import ctypes
import os
import re
import subprocess
import types

import pytest
import torch

from conftest import ROOT
from helpers import cfg_dict


def _header():
    text = open(os.path.join(ROOT, "include", "ytvln.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_gelu_fwd_is_declared_exported_and_bound():
    """Header, export table and ctypes table carry ytvln_gelu_fwd_f32 with one signature; ytvln_act_fwd_* keeps its own (swish only)."""
    from ytvln import _build, _lib
    _build.build(verbose=False)
    m = re.search(r"\bint\s+ytvln_gelu_fwd_f32\s*\(([^)]*)\)\s*;", _header())
    assert m, "ytvln_gelu_fwd_f32 is not declared in ytvln.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const float* z", "float* h", "int64_t n", "void* stream"], args
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in exported.splitlines() if " T " in l}
    assert "ytvln_gelu_fwd_f32" in exported, "ytvln_gelu_fwd_f32 is not exported"
    assert _lib.SIGNATURES["ytvln_gelu_fwd_f32"] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    assert _lib.SIGNATURES["ytvln_act_fwd_f32"] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    assert re.search(r"#define\s+YTVLN_ABI_VERSION\s+2\b", _header()) and _lib.ABI_VERSION == 2          # an added symbol, no changed one


def test_gelu_fwd_argument_checks():
    """No GPU work: an empty problem succeeds (also with NULL pointers: an empty tensor has no address), a negative count and a NULL pointer
    with n > 0 are rejected and ytvln_last_error() names the function."""
    from ytvln import _lib
    lib = _lib.load()
    assert lib.ytvln_gelu_fwd_f32(16, 16, 0, None) == 0
    assert lib.ytvln_gelu_fwd_f32(None, None, 0, None) == 0
    for bad in ((16, 16, -1), (None, 16, 4), (16, None, 4), (None, None, 1)):
        assert lib.ytvln_gelu_fwd_f32(*bad, None) != 0, bad
        assert b"gelu_fwd" in lib.ytvln_last_error(), (bad, lib.ytvln_last_error())
    with pytest.raises(RuntimeError, match="ytvln_gelu_fwd_f32 failed.*gelu_fwd"):
        _lib.call("ytvln_gelu_fwd_f32", None, 16, 4, None)


class _State:
    """Stand-in for ops.DropoutState: the site counter and its accessor, nothing on a device."""

    def __init__(self, site=0):
        self._site = site

    def next_site(self):
        self._site += 1
        return self._site


def test_replay_rewinds_restores_and_nests():
    from ytvln import vilbert as V
    R = V._Runtime
    before = R.drop
    try:
        first = _State()
        R.drop = first
        assert [first.next_site() for _ in range(5)] == [1, 2, 3, 4, 5]          # a forward: a segment entered at counter 2 took sites 3 and 4
        other = _State(40)
        R.drop = other          # another forward has replaced the state since
        with V._replay_drop(first, 2) as st:
            assert st is first and R.drop is first, "the recorded object is installed, not the state of the moment"
            assert [R.drop.next_site(), R.drop.next_site()] == [3, 4], "the replay hands out the sites of the first run"
        assert R.drop is other and other._site == 40 and first._site == 5, "previous state back, the recorded counter where it was"
        # the body raises: everything is restored all the same
        with pytest.raises(KeyError):
            with V._replay_drop(first, 0):
                assert R.drop.next_site() == 1
                raise KeyError("boom")
        assert R.drop is other and first._site == 5
        # nested: the inner replay of the same object rewinds further back and leaves the outer one's position intact
        with V._replay_drop(first, 2):
            assert R.drop.next_site() == 3
            with V._replay_drop(first, 0):
                assert [R.drop.next_site(), R.drop.next_site()] == [1, 2]
                with V._replay_drop(other, 7):
                    assert R.drop is other and R.drop.next_site() == 8
                assert R.drop is first and other._site == 40
            assert R.drop is first and R.drop.next_site() == 4
        assert R.drop is other and first._site == 5
        # nothing recorded (a segment that ran without dropout state): the replay installs None and restores
        with V._replay_drop(None, 0) as st:
            assert st is None and R.drop is None
        assert R.drop is other
    finally:
        R.drop = before


def _config(**args_fields):
    from ytvln.vilbert import BertConfig
    cfg = BertConfig(**cfg_dict("micro.json"))
    if args_fields is not None:
        cfg.args = types.SimpleNamespace(model_name="vilbert", **args_fields)
    return cfg


def test_bert_model_takes_the_attribute_from_config_args():
    from ytvln.vilbert import BertConfig, BertEncoder, BertModel
    assert BertEncoder.recompute == "none" and "recompute" not in BertConfig.__dataclass_fields__          # an attribute, not a config field
    with pytest.raises(TypeError):
        BertConfig(**cfg_dict("micro.json", recompute="layer"))          # the config stays the reference's strict dataclass
    assert BertModel(BertConfig(**cfg_dict("micro.json"))).encoder.recompute == "none"          # no args object
    assert BertModel(_config(max_grad_norm=1.0)).encoder.recompute == "none"                      # an args object without the field
    for tier in ("none", "ffn", "layer"):
        assert BertModel(_config(recompute=tier)).encoder.recompute == tier
    plain, on = BertModel(_config()), BertModel(_config(recompute="layer"))
    assert list(plain.state_dict()) == list(on.state_dict())
    assert [n for n, _ in plain.named_parameters()] == [n for n, _ in on.named_parameters()]
    on.encoder.recompute = "ffn"          # a plain attribute: set after construction like use_co_attention_mask
    assert on.encoder.recompute == "ffn" and plain.encoder.recompute == "none"


def test_guards_that_need_no_device():
    from ytvln import distributed as D, ops, vilbert as V
    model = V.BertModel(_config(recompute="rows"))          # the value is checked at the next forward, before any launch
    with pytest.raises(ValueError, match="recompute"):
        model.encoder(None, None, None, None)
    with pytest.raises(ValueError, match="recompute"):
        model.eval().encoder(None, None, None, None)
    model.train()
    model.encoder.recompute = "layer"
    with pytest.raises(NotImplementedError, match="recompute.*output_all_attention_masks"):
        model.encoder(None, None, None, None, output_all_attention_masks=True)
    for tier in ("ffn", "layer"):
        model.encoder.recompute = tier
        model.encoder.cut_after = frozenset({"c0"})
        with pytest.raises(NotImplementedError, match="recompute.*cut_after"):
            model.encoder(None, None, None, None)
        model.encoder.cut_after = frozenset()
        with pytest.raises(NotImplementedError, match="recompute"):          # refused before the optimizer or the step function is touched
            D.GraphedTrainStep(model, None, None)
    assert V._Runtime.ffn_recompute is False, "a refused forward leaves nothing installed"
    # inert where nothing is kept for a backward: eval mode and torch.no_grad() resolve every tier to "none"
    model.encoder.recompute = "layer"
    with torch.no_grad():
        assert model.encoder._recompute_tier(True) == "none"
    assert model.eval().encoder._recompute_tier(True) == "none" and model.train().encoder._recompute_tier(False) == "layer"
    # bf16 hidden states: the FFN tier is refused by the wrapper itself, with the way out in the message
    x = torch.zeros(2, 4, dtype=torch.bfloat16)
    w = torch.zeros(4, 4)
    for fn in (ops.ffn, ops.ffn_res):
        with pytest.raises(NotImplementedError, match='recompute = "ffn".*"layer"'):
            fn(x, w, None, w, None, recompute_h=True)
