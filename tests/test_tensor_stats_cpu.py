"""CPU: the per-tensor gradient / weight statistics of the arena AdamW step (AdamW.tensor_stats) -- everything that needs no device: the
two entry points are declared, exported and bound as declared; bad arguments are rejected before the GPU is touched; `tensor_stats` is a
plain attribute (default off, not in param_groups / defaults / state_dict) that get_optimization sets from `args.tensor_stats`; anything but
a bool raises when the step is taken, before the CPU-tensor error can; the accessors raise before any step."""
import subprocess

import pytest
import torch
from torch import nn

from test_abi import ctype_of, header_decls

NEW = {
    "ytvln_tensor_stats_stage1": ["const float* p", "const void* g", "int g_dtype", "const void* chunks", "int nchunks", "float* partials",
                                  "int32_t* bad", "void* stream"],
    "ytvln_tensor_stats_stage2": ["const float* partials", "const int32_t* bad", "const int32_t* tensor_first", "const int32_t* rec_tensor",
                                  "int ntensors", "float grad_scale", "float* stats", "int64_t* counts", "void* stream"],
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

    ok1 = dict(p=A, g=A, dt=_lib.DT_F32, ch=A, n=1, part=B, bad=B)

    def stage1(**kw):
        a = dict(ok1, **kw)
        return lib.ytvln_tensor_stats_stage1(a["p"], a["g"], a["dt"], a["ch"], a["n"], a["part"], a["bad"], None)
    for k in ("p", "g", "ch", "part", "bad"):
        assert stage1(**{k: None}) != 0 and b"null" in err(), k
    for k in ("p", "g", "part"):
        assert stage1(**{k: A + 8}) != 0 and b"aligned" in err(), k
    assert stage1(bad=B + 4) != 0 and b"aligned" in err()
    for dt in (_lib.DT_F64, _lib.DT_I64, _lib.DT_U8, -1, 17):
        assert stage1(dt=dt) != 0 and b"dtype" in err()
    assert stage1(n=-1) != 0 and b"nchunks" in err()
    assert stage1(n=0) == 0 and stage1(n=0, dt=_lib.DT_BF16, bad=B + 8) == 0          # empty table: no-op

    ok2 = dict(part=A, bad=A, first=A, rec=A, nt=1, gs=1.0, stats=B, counts=B)

    def stage2(**kw):
        a = dict(ok2, **kw)
        return lib.ytvln_tensor_stats_stage2(a["part"], a["bad"], a["first"], a["rec"], a["nt"], a["gs"], a["stats"], a["counts"], None)
    for k in ("part", "bad", "first", "rec", "stats", "counts"):
        assert stage2(**{k: None}) != 0 and b"null" in err(), k
    assert stage2(part=A + 8) != 0 and b"aligned" in err()
    assert stage2(stats=B + 8) != 0 and b"aligned" in err()
    assert stage2(bad=A + 4) != 0 and b"aligned" in err()
    assert stage2(counts=B + 4) != 0 and b"aligned" in err()
    assert stage2(nt=-2) != 0 and b"ntensors" in err()
    assert stage2(nt=0) == 0 and stage2(nt=0, counts=B + 8) == 0
    with pytest.raises(RuntimeError, match="ytvln_tensor_stats_stage1 failed"):
        _lib.call("ytvln_tensor_stats_stage1", A, A, _lib.DT_F64, A, 1, B, B, None)


def _args(**kw):
    from helpers import args_ns
    return args_ns(**kw)


def test_default_is_off():
    from ytvln.optimization import AdamW
    opt = AdamW([nn.Parameter(torch.zeros(4))], lr=1e-3)
    assert opt.tensor_stats is False and opt.stats_setting() is False
    assert opt.stats_buffers() is None          # no arena yet: nothing to allocate


def test_get_optimization_sets_the_attribute_from_args_tensor_stats():
    from ytvln.vilbert_init import get_optimization
    model = nn.Linear(4, 4)
    opt, _, _, _ = get_optimization(_args(), model, 10, None)          # an argument object without the field: off
    assert opt.tensor_stats is False
    opt, _, _, _ = get_optimization(_args(tensor_stats=True), model, 10, None)
    assert opt.tensor_stats is True and opt.stats_setting() is True
    opt, _, _, _ = get_optimization(_args(tensor_stats=False), model, 10, None)
    assert opt.tensor_stats is False
    assert opt.max_grad_norm is None and opt.skip_nonfinite is False and opt.trust_ratio is False and opt.ema_decay is None


def test_attribute_is_not_a_constructor_argument_nor_optimizer_state():
    from ytvln.optimization import AdamW
    with pytest.raises(TypeError):
        AdamW([nn.Parameter(torch.zeros(4))], lr=1e-3, tensor_stats=True)
    ps = [nn.Parameter(torch.zeros(4)), nn.Parameter(torch.zeros(3))]
    plain = AdamW(ps, lr=1e-3)
    on = AdamW(ps, lr=1e-3)
    on.tensor_stats = True
    sa, sb = plain.state_dict(), on.state_dict()
    assert sa.keys() == sb.keys() and sa["state"].keys() == sb["state"].keys()
    assert [sorted(g) for g in sa["param_groups"]] == [sorted(g) for g in sb["param_groups"]]
    assert repr(sa) == repr(sb)
    assert plain.defaults == on.defaults and "tensor_stats" not in on.defaults
    assert all("tensor_stats" not in g for g in on.param_groups)


def test_accessors_raise_before_any_step():
    from ytvln.optimization import AdamW
    model = nn.Linear(4, 4)
    opt = AdamW(model.parameters(), lr=1e-3)
    opt.tensor_stats = True
    with pytest.raises(RuntimeError, match="no step has been taken"):
        opt.tensor_stats_report()
    with pytest.raises(RuntimeError, match="no step has been taken"):
        opt.tensor_names(model)
    with pytest.raises(RuntimeError, match="no step has been taken"):
        opt.nonfinite_tensors(model)


@pytest.mark.parametrize("bad", [1, "yes", None])
def test_anything_but_a_bool_raises_when_the_step_is_taken(bad):
    from ytvln.optimization import AdamW
    p = nn.Parameter(torch.zeros(4))
    opt = AdamW([p], lr=1e-3)
    opt.tensor_stats = bad          # plain attribute: assignment itself never raises
    p.grad = torch.ones(4)          # a CPU tensor: with a valid setting the step fails later, with a RuntimeError (there is no CPU path)
    with pytest.raises(ValueError, match="tensor_stats"):
        opt.step()
    with pytest.raises(ValueError, match="tensor_stats"):
        opt.stats_setting()
    opt.tensor_stats = True
    with pytest.raises(RuntimeError):
        opt.step()


def test_prepare_replay_refuses_a_setting_changed_after_a_capture():
    """A captured step bakes the setting in: the host-side check needs no device."""
    from ytvln.optimization import AdamW, CaptureSettings
    opt = AdamW([nn.Parameter(torch.zeros(4))], lr=1e-3)
    opt._launch = []                      # (no launch classes: prepare_replay uploads nothing)
    opt.tensor_stats = True
    opt.prepare_replay()                  # nothing captured yet: any setting goes
    opt._captured = CaptureSettings(stats=False)         # as a capture with the feature off leaves it
    with pytest.raises(RuntimeError, match="capture the step again"):
        opt.prepare_replay()
    opt.tensor_stats = False
    opt.prepare_replay()
    opt._captured = CaptureSettings(stats=True)         # as a capture with it on leaves it
    with pytest.raises(RuntimeError, match="capture the step again"):
        opt.prepare_replay()
    opt.tensor_stats = True
    opt.prepare_replay()
