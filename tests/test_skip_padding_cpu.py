"""CPU: the host side of padding-free execution (BertModel.skip_padding) -- argument checks of the packed-row entry points, the capacity rule,
attribute validation, the refusal of CPU tensors, and a numpy restatement of what ytvln_rows_plan must produce (the GPU test pins the kernel to
torch.nonzero; this file pins the statement itself)."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

from helpers import ZERO_DROP, cfg_dict


def plan_ref(flags, capacity):
    """include/ytvln.h, ytvln_rows_plan, in numpy: (pack_idx[capacity], unpack_idx[rows], counts[2])."""
    flags = np.asarray(flags).reshape(-1) != 0
    where = np.nonzero(flags)[0]                       # ascending: packed row j is the j-th flagged row
    pack = np.full(capacity, -1, np.int64)
    fit = where[:capacity]
    pack[:len(fit)] = fit
    unpack = np.full(flags.size, -1, np.int64)
    unpack[fit] = np.arange(len(fit))
    return pack, unpack, np.array([len(where), max(len(where) - capacity, 0)], np.int64)


def test_plan_statement_is_a_partial_bijection():
    rs = np.random.RandomState(0)
    for rows, cap in ((1, 1), (65, 10), (65, 65), (1025, 700), (300, 1)):
        flags = rs.rand(rows) < 0.5
        pack, unpack, counts = plan_ref(flags, cap)
        n = int(flags.sum())
        assert counts[0] == n and counts[1] == max(n - cap, 0)
        live = pack[pack >= 0]
        assert len(live) == min(n, cap) and np.all(np.diff(live) > 0) and np.all(flags[live])          # stable, flagged rows only
        assert np.array_equal(unpack[live], np.arange(len(live)))                                      # unpack inverts pack ...
        assert np.array_equal(pack[unpack[unpack >= 0]], np.nonzero(unpack >= 0)[0])                   # ... and pack inverts unpack
        assert np.all(unpack[~flags] == -1) and int((unpack >= 0).sum()) == len(live)
        # pack and unpack as matrices are each other's transpose: the mover with one index array is the adjoint of the mover with the other
        P = np.zeros((cap, rows)); P[np.nonzero(pack >= 0)[0], live] = 1
        U = np.zeros((rows, cap)); U[np.nonzero(unpack >= 0)[0], unpack[unpack >= 0]] = 1
        assert np.array_equal(P.T, U)


def test_entry_points_reject_bad_arguments_without_touching_a_device():
    from ytvln import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)          # a non-null pointer that is never dereferenced: every call below fails in the argument checks
    assert lib.ytvln_rows_plan(None, 4, 4, one, one, one, None) != 0 and b"null" in lib.ytvln_last_error()
    assert lib.ytvln_rows_plan(one, 4, 4, one, None, one, None) != 0 and b"null" in lib.ytvln_last_error()
    assert lib.ytvln_rows_plan(one, -1, 4, one, one, one, None) != 0 and b"rows_plan" in lib.ytvln_last_error()
    assert lib.ytvln_rows_plan(one, 4, -2, one, one, one, None) != 0 and b"rows_plan" in lib.ytvln_last_error()
    for name in ("ytvln_rows_move_f32", "ytvln_rows_move_bf16"):
        fn = getattr(lib, name)
        assert fn(None, 8, 4, one, 2, 8, one, 8, None) != 0 and b"null" in lib.ytvln_last_error()
        assert fn(one, 8, 4, None, 2, 8, one, 8, None) != 0 and b"null" in lib.ytvln_last_error()
        assert fn(one, 8, 4, one, 2, 8, None, 8, None) != 0 and b"null" in lib.ytvln_last_error()
        assert fn(one, 8, 4, one, -1, 8, one, 8, None) != 0 and b"negative" in lib.ytvln_last_error()
        assert fn(one, 8, -4, one, 2, 8, one, 8, None) != 0 and b"negative" in lib.ytvln_last_error()
        assert fn(one, 8, 4, one, 2, 0, one, 8, None) != 0                                        # width >= 1
        assert fn(one, 4, 4, one, 2, 8, one, 8, None) != 0 and b"leading" in lib.ytvln_last_error()
        assert fn(None, 8, 4, None, 0, 8, None, 8, None) == 0                                     # out_rows = 0: nothing to do, no launch
    with pytest.raises(RuntimeError, match="ytvln_rows_plan failed"):
        _lib.call("ytvln_rows_plan", None, 4, 4, None, None, None, None)


def test_capacity_rule():
    from ytvln import ops
    for rows, frac in ((4480, 0.7), (16128, 0.5), (16128, 1.0), (100, 0.5), (576, 0.4), (576, 1e-6), (257, 1.0), (18432, 0.45)):
        want = min(rows, int(math.ceil(frac * rows / 256)) * 256)
        got = ops.rows_capacity(rows, frac)
        assert got == want and 1 <= got <= rows and (got == rows or got % 256 == 0), (rows, frac, got)
    assert ops.rows_capacity(4480, 0.7) == 3328 and ops.rows_capacity(100, 0.5) == 100 and ops.rows_capacity(576, 0.4) == 256


def _model(**args_over):
    from ytvln.vilbert import BertConfig, BertModel
    cfg = BertConfig(**cfg_dict("micro.json", **ZERO_DROP))
    if args_over:
        cfg.args = types.SimpleNamespace(**args_over)
    return BertModel(cfg)


def test_attribute_default_config_field_and_validation():
    from ytvln import vilbert as V
    assert V.BertModel.skip_padding is None
    m = _model()
    assert m.skip_padding is None and m.padding_overflow is None
    assert "padding_overflow" not in m.state_dict() and not any("padding" in k for k in m.state_dict())
    assert _model(skip_padding=0.5).skip_padding == 0.5 and _model(recompute="none").skip_padding is None
    assert V._skip_padding_spec(None) is None
    assert V._skip_padding_spec(0.5) == (0.5, 0.5) and V._skip_padding_spec(1) == (1, 1) and V._skip_padding_spec((0.7, 0.5)) == (0.7, 0.5)
    assert V._skip_padding_spec("exact") == ("exact", "exact")
    for bad in (0.0, -0.5, 1.5, True, "yes", (0.5,), (0.5, 0.5, 0.5), (0.5, "exact"), (0.5, 0.0), [0.5, 2.0], {"t": 0.5}):
        with pytest.raises(ValueError, match="BertModel.skip_padding"):
            V._skip_padding_spec(bad)


def test_cpu_tensors_raise_no_fallback():
    from ytvln import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rows_plan(torch.ones(4, 8), 16)
    plan = ops.RowsPlan(torch.zeros(4, dtype=torch.int64), torch.zeros(8, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), 8, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rows_pack(torch.zeros(8, 4), plan)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rows_unpack(torch.zeros(4, 4), plan)
    m = _model()
    m.skip_padding = 0.5
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 4, dtype=torch.long), torch.zeros(2, 3, 16), torch.zeros(2, 3, 12), attention_mask=torch.ones(2, 4),
          image_attention_mask=torch.ones(2, 3))
