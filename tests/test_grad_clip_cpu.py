"""CPU: global gradient-norm clipping (AdamW.max_grad_norm / skip_nonfinite) -- everything that needs no device: the three entry points
are declared, exported and bound as declared; bad arguments are rejected before the GPU is touched; the two attributes are plain
attributes (defaults off, not in param_groups / defaults / state_dict), set by get_optimization from `args`; bad values raise; nothing is
allocated while the feature is off."""
import ctypes
import math
import subprocess
import types

import pytest
import torch
from torch import nn

from test_abi import ctype_of, header_decls

NEW = {
    "ytvln_grad_sumsq": ["const void* g", "int dtype", "const void* chunks", "int nchunks", "float* partials", "void* stream"],
    "ytvln_grad_clip_coef": ["const float* partials", "int64_t n", "float grad_scale", "float max_norm", "int skip_nonfinite", "float* clip",
                             "void* stream"],
    "ytvln_adamw_clip": ["float* p", "const void* g", "int g_dtype", "float* m", "float* v", "uint16_t* p_bf16", "const void* chunks",
                         "int nchunks", "const float* hyper", "float grad_scale", "const float* clip", "void* stream"],
}


def test_entry_points_declared_exported_and_bound():
    from ytvln import _lib
    lib = _lib.load()
    decls = header_decls()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in exported.splitlines() if " T " in l}
    for name, args in NEW.items():
        assert name in decls, f"{name} is not declared in include/ytvln.h"
        ret, got = decls[name]
        assert ret == "int"
        assert [" ".join(a.split()) for a in got] == args, (name, got)
        assert name in exported and hasattr(lib, name)
        assert _lib.SIGNATURES[name] == [ctype_of(a) for a in args]
    assert lib.ytvln_version() == _lib.ABI_VERSION == 2          # additive: no bump


def test_bad_arguments_are_rejected_without_touching_the_gpu():
    """Pointers here are made-up addresses: every call must fail in its argument checks (a launch would fault)."""
    from ytvln import _lib
    lib = _lib.load()
    A, B = 0x10000, 0x20000          # 16-byte aligned
    err = lambda: lib.ytvln_last_error()          # noqa: E731
    # grad_sumsq
    assert lib.ytvln_grad_sumsq(None, _lib.DT_F32, A, 1, B, None) != 0 and b"null" in err()
    assert lib.ytvln_grad_sumsq(A, _lib.DT_F32, None, 1, B, None) != 0 and b"null" in err()
    assert lib.ytvln_grad_sumsq(A, _lib.DT_F32, A, 1, None, None) != 0 and b"null" in err()
    assert lib.ytvln_grad_sumsq(A + 4, _lib.DT_F32, A, 1, B, None) != 0 and b"aligned" in err()
    for dt in (_lib.DT_F64, _lib.DT_I64, _lib.DT_U8, 17):
        assert lib.ytvln_grad_sumsq(A, dt, A, 1, B, None) != 0 and b"dtype" in err()
    assert lib.ytvln_grad_sumsq(A, _lib.DT_F32, A, 0, B, None) == 0          # empty table: no-op
    assert lib.ytvln_grad_sumsq(A, _lib.DT_BF16, A, -3, B, None) == 0
    # grad_clip_coef
    assert lib.ytvln_grad_clip_coef(A, 4, 1.0, 1.0, 0, None, None) != 0 and b"null" in err()
    assert lib.ytvln_grad_clip_coef(None, 4, 1.0, 1.0, 0, B, None) != 0 and b"null" in err()
    assert lib.ytvln_grad_clip_coef(A, -1, 1.0, 1.0, 0, B, None) != 0
    for bad in (0.0, -1.0, float("nan"), -float("inf")):
        assert lib.ytvln_grad_clip_coef(A, 4, 1.0, bad, 0, B, None) != 0 and b"max_norm" in err(), bad
    # adamw_clip
    ok = dict(p=A, g=A, dt=_lib.DT_F32, m=A, v=A, pb=None, ch=A, n=1, hy=A, gs=1.0, clip=B)

    def adamw(**kw):
        a = dict(ok, **kw)
        return lib.ytvln_adamw_clip(a["p"], a["g"], a["dt"], a["m"], a["v"], a["pb"], a["ch"], a["n"], a["hy"], a["gs"], a["clip"], None)
    for k in ("p", "g", "m", "v", "ch", "hy", "clip"):
        assert adamw(**{k: None}) != 0 and b"null" in err(), k
    for k in ("p", "g", "m", "v", "pb"):
        assert adamw(**{k: A + 8}) != 0 and b"aligned" in err(), k
    for dt in (_lib.DT_F64, _lib.DT_I64, _lib.DT_U8, -1):
        assert adamw(dt=dt) != 0 and b"dtype" in err()
    assert adamw(n=0) == 0 and adamw(n=-1) == 0
    with pytest.raises(RuntimeError, match="ytvln_grad_clip_coef failed"):
        _lib.call("ytvln_grad_clip_coef", A, 4, 1.0, 0.0, 0, B, None)


def _args(**kw):
    from helpers import args_ns
    return args_ns(**kw)


def test_get_optimization_sets_the_attributes_from_args():
    from ytvln.vilbert_init import get_optimization
    model = nn.Linear(4, 4)
    opt, _, _, _ = get_optimization(_args(), model, 10, None)
    assert opt.max_grad_norm is None and opt.skip_nonfinite is False and opt.clip_settings() is None
    a = _args()
    a.max_grad_norm, a.skip_nonfinite_grads = 1.5, 1
    opt, _, _, _ = get_optimization(a, model, 10, None)
    assert opt.max_grad_norm == 1.5 and opt.skip_nonfinite is True and opt.clip_settings() == (1.5, True)
    a = _args()
    a.skip_nonfinite_grads = True
    opt, _, _, _ = get_optimization(a, model, 10, None)
    assert opt.max_grad_norm is None and opt.clip_settings() == (math.inf, True)          # measure and skip, never clip


def test_attributes_are_not_constructor_arguments_nor_optimizer_state():
    from ytvln.optimization import AdamW
    with pytest.raises(TypeError):
        AdamW([nn.Parameter(torch.zeros(4))], lr=1e-3, max_grad_norm=1.0)
    ps = [nn.Parameter(torch.zeros(4)), nn.Parameter(torch.zeros(3))]
    plain = AdamW(ps, lr=1e-3)
    on = AdamW(ps, lr=1e-3)
    on.max_grad_norm, on.skip_nonfinite = 1.0, True
    sa, sb = plain.state_dict(), on.state_dict()
    assert sa.keys() == sb.keys() and sa["state"].keys() == sb["state"].keys()
    assert [sorted(g) for g in sa["param_groups"]] == [sorted(g) for g in sb["param_groups"]]
    assert repr(sa) == repr(sb)
    assert "max_grad_norm" not in on.defaults and "skip_nonfinite" not in on.defaults
    assert all("max_grad_norm" not in g and "skip_nonfinite" not in g for g in on.param_groups)


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), "1.0", True, [1.0], torch.tensor(1.0)])
def test_bad_values_raise_when_the_step_is_taken(bad):
    from ytvln.optimization import AdamW
    p = nn.Parameter(torch.zeros(4))
    opt = AdamW([p], lr=1e-3)
    opt.max_grad_norm = bad          # plain attribute: assignment itself never raises
    p.grad = torch.ones(4)
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt.step()
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt.clip_settings()


@pytest.mark.parametrize("good,want", [(1, (1.0, False)), (0.25, (0.25, False)), (float("inf"), (math.inf, False)), (None, None)])
def test_good_values(good, want):
    from ytvln.optimization import AdamW
    opt = AdamW([nn.Parameter(torch.zeros(4))], lr=1e-3)
    opt.max_grad_norm = good
    assert opt.clip_settings() == want


def test_adamw_allocates_no_clip_buffers_by_default():
    from ytvln.optimization import AdamW
    opt = AdamW([nn.Parameter(torch.zeros(4))], lr=1e-3)
    assert opt.max_grad_norm is None and opt.skip_nonfinite is False
    assert opt.clip_buffers() is None and opt.skipped_steps() == 0          # no arena yet: nothing to allocate, nothing skipped
    with pytest.raises(RuntimeError, match="no step has been taken"):
        opt.grad_norm()
    st = opt.state_dict()["state"]
    assert "partials" not in st and "clip" not in st


def test_prepare_replay_refuses_settings_changed_after_a_capture():
    """A captured step bakes the settings in: the host-side check needs no device."""
    from ytvln.optimization import AdamW, CaptureSettings
    opt = AdamW([nn.Parameter(torch.zeros(4))], lr=1e-3)
    opt._launch = []                      # (no launch classes: prepare_replay uploads nothing)
    opt.prepare_replay()                  # nothing captured yet: any setting goes
    opt._captured = CaptureSettings(clip=None)      # as a capture with the feature off leaves it
    opt.prepare_replay()
    opt.max_grad_norm = 1.0
    with pytest.raises(RuntimeError, match="capture the step again"):
        opt.prepare_replay()
    opt._captured = CaptureSettings(clip=(1.0, False))     # as a capture with max_grad_norm = 1 leaves it
    opt.prepare_replay()
    opt.max_grad_norm = 2.0
    with pytest.raises(RuntimeError, match="capture the step again"):
        opt.prepare_replay()
    opt.max_grad_norm, opt.skip_nonfinite = 1.0, True
    with pytest.raises(RuntimeError, match="capture the step again"):
        opt.prepare_replay()
