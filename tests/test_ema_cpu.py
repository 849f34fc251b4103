"""CPU: the EMA of the weights of the arena AdamW step (AdamW.ema_decay / ema_warmup / ema_updates; ytvln_ema_update, ytvln_ema_swap) --
everything that needs no device: the validator, the weight arithmetic, get_optimization, the attributes' absence from state_dict, the
launch sequence of a step followed with `ops.call` stubbed (the technique of tests/test_attn_dbias_cpu.py), the host-side checks of both
entry points, and the host-side refusals (a changed on / off after a capture, stepping while swapped)."""
import math
import subprocess

import numpy as np
import pytest
import torch
from torch import nn

from test_abi import ctype_of, header_decls

NEW = {
    "ytvln_ema_update": ["const float* p", "float* e", "const void* chunks", "int nchunks", "const float* hyper", "const float* clip",
                         "void* stream"],
    "ytvln_ema_swap": ["float* p", "float* e", "uint16_t* p_bf16", "const void* chunks", "int nchunks", "void* stream"],
}


def _opt(**attrs):
    from ytvln.optimization import AdamW
    opt = AdamW([nn.Parameter(torch.zeros(4))], lr=1e-3)
    for k, v in attrs.items():
        setattr(opt, k, v)
    return opt


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


# ---- 1. the validator ---------------------------------------------------------------------------------------------------------------------
def test_setting_is_off_by_default_and_for_none():
    opt = _opt()
    assert opt.ema_decay is None and opt.ema_warmup is False and opt.ema_updates == 0
    assert opt.ema_setting() is None and opt.ema_weight() == 0.0
    assert _opt(ema_decay=None, ema_warmup=True).ema_setting() is None
    assert _opt(ema_decay=0.999).ema_setting() == (0.999, False)
    assert _opt(ema_decay=0.5, ema_warmup=True).ema_setting() == (0.5, True)
    assert _opt(ema_decay=np.float32(0.75)).ema_setting() == (0.75, False)
    assert opt.ema_buffers() is None and opt.ema_parameters() == {}          # no arena yet: nothing to allocate


@pytest.mark.parametrize("bad", [True, False, 0, 1, 0.0, 1.0, 1.5, -0.1, float("nan"), float("inf"), "0.9", [0.9], torch.tensor(0.9)])
def test_a_bad_decay_raises_when_the_step_is_taken(bad):
    opt = _opt()
    p = opt.param_groups[0]["params"][0]
    opt.ema_decay = bad          # plain attribute: assignment itself never raises
    p.grad = torch.ones(4)
    with pytest.raises(ValueError, match="ema_decay"):
        opt.ema_setting()
    with pytest.raises(ValueError, match="ema_decay"):
        opt.step()
    opt._launch = []
    with pytest.raises(ValueError, match="ema_decay"):
        opt.prepare_replay()


@pytest.mark.parametrize("bad", [1, 0, "True", None, np.bool_(True), torch.tensor(True)])
@pytest.mark.parametrize("decay", [None, 0.9])
def test_a_non_bool_warmup_raises_when_the_step_is_taken(bad, decay):
    opt = _opt(ema_decay=decay, ema_warmup=bad)
    opt.param_groups[0]["params"][0].grad = torch.ones(4)
    with pytest.raises(ValueError, match="ema_warmup"):
        opt.ema_setting()
    with pytest.raises(ValueError, match="ema_warmup"):
        opt.step()


# ---- 2. the weight ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("n", [0, 1, 9, 10 ** 6])
def test_weight_is_one_minus_the_effective_decay_rounded_once_to_fp32(warm, n):
    d = 0.9999
    opt = _opt(ema_decay=d, ema_warmup=warm)
    want = np.float32(1.0 - (min(d, (1.0 + n) / (10.0 + n)) if warm else d))          # double arithmetic, one rounding
    got = opt.ema_weight(n)
    assert isinstance(got, float) and np.float32(got) == want and float(np.float32(got)) == got, (got, want)
    opt.ema_updates = n                                                                # the count the optimizer keeps is the default n
    assert opt.ema_weight() == got
    if warm and n < 10 ** 6:
        assert got > float(np.float32(1.0 - d))                                        # warm-up: a shorter memory early on
    if warm and n == 0:
        assert got == float(np.float32(0.9))
    if not warm or n == 10 ** 6:
        assert got == float(np.float32(1.0 - d))


# ---- 3. get_optimization --------------------------------------------------------------------------------------------------------------------
def test_get_optimization_sets_the_attributes_from_args():
    from helpers import args_ns
    from ytvln.vilbert_init import get_optimization
    model = nn.Linear(4, 4)
    opt, _, _, _ = get_optimization(args_ns(), model, 10, None)          # an argument object without the fields: off
    assert opt.ema_decay is None and opt.ema_warmup is False and opt.ema_setting() is None
    opt, _, _, _ = get_optimization(args_ns(ema_decay=0.999), model, 10, None)
    assert opt.ema_decay == 0.999 and opt.ema_warmup is False and opt.ema_setting() == (0.999, False)
    opt, _, _, _ = get_optimization(args_ns(ema_decay=0.99, ema_warmup=True), model, 10, None)
    assert opt.ema_setting() == (0.99, True)
    opt, _, _, _ = get_optimization(args_ns(ema_decay=None), model, 10, None)
    assert opt.ema_setting() is None
    assert opt.max_grad_norm is None and opt.skip_nonfinite is False and opt.trust_ratio is False


def test_attributes_are_not_constructor_arguments_nor_optimizer_state():
    from ytvln.optimization import AdamW
    for kw in ({"ema_decay": 0.9}, {"ema_warmup": True}):
        with pytest.raises(TypeError):
            AdamW([nn.Parameter(torch.zeros(4))], lr=1e-3, **kw)
    ps = [nn.Parameter(torch.zeros(4)), nn.Parameter(torch.zeros(3))]
    plain, on = AdamW(ps, lr=1e-3), AdamW(ps, lr=1e-3)
    on.ema_decay, on.ema_warmup, on.ema_updates = 0.9, True, 7
    sa, sb = plain.state_dict(), on.state_dict()
    assert sa.keys() == sb.keys() and repr(sa) == repr(sb)
    assert plain.defaults == on.defaults
    for k in ("ema_decay", "ema_warmup", "ema_updates"):
        assert k not in on.defaults and all(k not in g for g in on.param_groups)
    assert plain.ema_checkpoint(nn.Linear(2, 2)) is None          # feature off: nothing joins a checkpoint


# ---- 4. the launch sequence, `ops.call` stubbed -----------------------------------------------------------------------------------------------
class _Event:
    def record(self):
        pass

    def synchronize(self):
        pass


UPDATES = {"ytvln_adamw_f32", "ytvln_adamw_f32_bf16copy", "ytvln_adamw_f32_gbf16", "ytvln_adamw_clip", "ytvln_lamb_stage2"}


def _stubbed(monkeypatch, **attrs):
    """An AdamW over two parameter groups whose arenas and launch classes are hand-made CPU tensors (the layout _build_arena /
    _build_launch produce); every ops.call is recorded instead of run.  -> (optimizer, the recorded calls)."""
    import struct
    from ytvln import ops
    from ytvln.optimization import AdamW, lamb_tables, new_arena
    seen = []
    monkeypatch.setattr(ops, "call", lambda name, *a: seen.append((name, a)))
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "_check", lambda *a, **k: None)
    monkeypatch.setattr(ops, "_check_i32", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    ps = [nn.Parameter(torch.full((5,), 1.0)), nn.Parameter(torch.full((8,), 2.0))]
    opt = AdamW([{"params": [ps[0]], "weight_decay": 0.01}, {"params": [ps[1]], "weight_decay": 0.0}], lr=1e-3)
    for k, v in attrs.items():
        setattr(opt, k, v)
    index = {id(ps[0]): (0, 5), id(ps[1]): (8, 8)}
    flat = {k: torch.zeros(16) for k in "pgmv"}
    flat["p"][0:5], flat["p"][8:16] = 1.0, 2.0
    opt._arena = new_arena(flat, index, [id(p) for p in ps])
    opt._written = set()
    opt._launch = []
    for gi, p in enumerate(ps):
        o, n = index[id(p)]
        first, rec = lamb_tables([(gi, n)])
        opt.state[p]["step"] = 0
        opt._launch.append(dict(group=gi, step=0, params=[p], n=1, rec0=gi, ntensors=1,
                                table=torch.frombuffer(bytearray(struct.pack("<qqff", o, n, 0.01 if gi == 0 else 0.0, 0.0)), dtype=torch.uint8),
                                tensor_first=torch.tensor(first, dtype=torch.int32), rec_tensor=torch.tensor(rec, dtype=torch.int32),
                                hyper=torch.zeros(8), ring=[torch.zeros(8) for _ in range(4)], events=[None] * 4, slot=0))
    return opt, seen


def _one_step(opt):
    opt._upload_hyper()
    opt._launch_kernels()


def test_feature_off_launches_nothing_new_and_uploads_a_zero_weight(monkeypatch):
    opt, seen = _stubbed(monkeypatch)
    for c in opt._launch:
        c["hyper"][6] = 123.0                                          # whatever was there
    _one_step(opt)
    names = [n for n, _ in seen]
    assert names == ["ytvln_adamw_f32", "ytvln_adamw_f32"], names
    assert not any(n.startswith("ytvln_ema_") for n in names)
    assert all(float(c["hyper"][6]) == 0.0 and float(c["hyper"][7]) == 0.0 for c in opt._launch)
    assert all(float(c["hyper"][4]) == np.float32(1e-3) for c in opt._launch)          # (the record was uploaded)
    assert opt._arena["ema"] is None and opt.ema_updates == 0


@pytest.mark.parametrize("extra,per_class", [
    ({}, ["ytvln_adamw_f32", "ytvln_ema_update"]),
    ({"max_grad_norm": 1.0}, ["ytvln_adamw_clip", "ytvln_ema_update"]),
    ({"trust_ratio": True}, ["ytvln_lamb_stage1", "ytvln_lamb_trust", "ytvln_lamb_stage2", "ytvln_ema_update"]),
    ({"trust_ratio": True, "skip_nonfinite": True}, ["ytvln_lamb_stage1", "ytvln_lamb_trust", "ytvln_lamb_stage2", "ytvln_ema_update"]),
])
def test_feature_on_exactly_one_ema_update_follows_each_update_launch(monkeypatch, extra, per_class):
    opt, seen = _stubbed(monkeypatch, ema_decay=0.9, ema_warmup=True, **extra)
    _one_step(opt)
    a = opt._arena
    names = [n for n, _ in seen if n not in ("ytvln_grad_sumsq", "ytvln_grad_clip_coef")]
    assert names == per_class * 2, names
    for i, (name, args) in enumerate(seen):
        if name in UPDATES:
            assert seen[i + 1][0] == "ytvln_ema_update", [n for n, _ in seen]
    calls = [args for name, args in seen if name == "ytvln_ema_update"]
    assert len(calls) == len(opt._launch) == sum(n in UPDATES for n, _ in seen)
    clip = a["clip"].data_ptr() if (extra.get("max_grad_norm") or extra.get("skip_nonfinite")) else None
    for c, args in zip(opt._launch, calls):          # (p, e, chunks, nchunks, hyper, clip, stream): the table and the record of ITS class
        assert args == (a["p"].data_ptr(), a["ema"].data_ptr(), c["table"].data_ptr(), c["n"], c["hyper"].data_ptr(), clip, 0)
    assert a["ema"].data_ptr() != a["p"].data_ptr() and torch.equal(a["ema"], a["p"])          # the shadow starts as a copy of the weights
    # the weight: warm-up at n = 0 is decay_eff = 0.1 -> min(0.9, 0.1); the count advanced once for the whole step
    assert all(float(c["hyper"][6]) == np.float32(1.0 - 0.1) for c in opt._launch)
    assert opt.ema_updates == 1
    opt.ema_warmup = False                                              # by value through the record: a changed setting is the next upload
    _one_step(opt)
    assert all(float(c["hyper"][6]) == np.float32(1.0 - 0.9) for c in opt._launch) and opt.ema_updates == 2
    opt.ema_decay = None                                                # off again: nothing launched, the slot goes back to 0
    del seen[:]
    _one_step(opt)
    assert not any(n.startswith("ytvln_ema_") for n, _ in seen)
    assert all(float(c["hyper"][6]) == 0.0 for c in opt._launch) and opt.ema_updates == 2


def test_swap_runs_over_every_launch_class_and_blocks_training_until_swapped_back(monkeypatch):
    opt, seen = _stubbed(monkeypatch, ema_decay=0.9)
    with pytest.raises(RuntimeError, match="no step has been taken"):
        opt.swap_ema()
    _one_step(opt)
    a = opt._arena
    a["pb"] = torch.zeros(16, dtype=torch.bfloat16)
    del seen[:]
    with opt.ema_weights():
        assert [n for n, _ in seen] == ["ytvln_ema_swap"] * 2
        for c, (_, args) in zip(opt._launch, seen):
            assert args == (a["p"].data_ptr(), a["ema"].data_ptr(), a["pb"].data_ptr(), c["table"].data_ptr(), c["n"], 0)
        for call in (opt.step, opt.prepare_replay, opt.capture_update, opt.launch_classes, lambda: opt.launch_tables([]),
                     lambda: opt.ema_state_dict(nn.Linear(2, 2)), lambda: opt.load_state_dict(opt.state_dict())):
            with pytest.raises(RuntimeError, match="swap"):
                call()
    assert [n for n, _ in seen] == ["ytvln_ema_swap"] * 4          # and back out
    opt.prepare_replay()


def test_prepare_replay_refuses_on_off_changed_after_a_capture_but_not_a_changed_decay():
    from ytvln.optimization import CaptureSettings
    opt = _opt()
    opt._launch = []                      # (no launch classes: prepare_replay uploads nothing)
    opt.ema_decay = 0.9
    opt.prepare_replay()                  # nothing captured yet: any setting goes
    opt._captured = CaptureSettings(ema=False)           # as a capture with the feature off leaves it
    with pytest.raises(RuntimeError, match="capture the step again"):
        opt.prepare_replay()
    opt.ema_decay = None
    opt.prepare_replay()
    opt._captured = CaptureSettings(ema=True)           # as a capture with it on leaves it
    with pytest.raises(RuntimeError, match="capture the step again"):
        opt.prepare_replay()
    n = opt.ema_updates
    for d, warm in ((0.9, False), (0.5, True), (0.999, False)):          # decay and warm-up travel by value: no recapture
        opt.ema_decay, opt.ema_warmup = d, warm
        opt.prepare_replay()
    assert opt.ema_updates == n + 3


# ---- 5. the host-side checks of the entry points ----------------------------------------------------------------------------------------------
def test_bad_arguments_are_rejected_without_touching_the_gpu():
    """Pointers here are made-up addresses: every call must fail in its argument checks (a launch would fault)."""
    from ytvln import _lib
    lib = _lib.load()
    A, B = 0x10000, 0x20000          # 16-byte aligned
    err = lambda: lib.ytvln_last_error()          # noqa: E731
    ok = dict(p=A, e=B, ch=A, n=1, hy=A, clip=None)

    def update(**kw):
        a = dict(ok, **kw)
        return lib.ytvln_ema_update(a["p"], a["e"], a["ch"], a["n"], a["hy"], a["clip"], None)
    for k in ("p", "e", "ch", "hy"):
        assert update(**{k: None}) < 0 and b"null" in err(), k
    for k in ("p", "e"):
        for d in (4, 8):
            assert update(**{k: A + d}) < 0 and b"aligned" in err(), k
    assert update(n=-1) < 0 and b"nchunks" in err()
    assert update(n=0) == 0 and update(n=0, clip=B) == 0          # empty table: no-op

    ok2 = dict(p=A, e=B, pb=None, ch=A, n=1)

    def swap(**kw):
        a = dict(ok2, **kw)
        return lib.ytvln_ema_swap(a["p"], a["e"], a["pb"], a["ch"], a["n"], None)
    for k in ("p", "e", "ch"):
        assert swap(**{k: None}) < 0 and b"null" in err(), k
    for k in ("p", "e", "pb"):
        assert swap(**{k: A + 8}) < 0 and b"aligned" in err(), k
    assert swap(n=-3) < 0 and b"nchunks" in err()
    assert swap(n=0) == 0 and swap(n=0, pb=B) == 0
    with pytest.raises(RuntimeError, match="ytvln_ema_update failed"):
        _lib.call("ytvln_ema_update", A, B, A, -1, A, None, None)
    with pytest.raises(RuntimeError, match="ytvln_ema_swap failed"):
        _lib.call("ytvln_ema_swap", A, None, None, A, 1, None)


def test_wrappers_refuse_cpu_tensors_no_fallback():
    from ytvln import ops
    z = torch.zeros(16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ema_update(z, z.clone(), torch.zeros(24, dtype=torch.uint8), 1, torch.zeros(8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ema_swap(z, z.clone(), torch.zeros(24, dtype=torch.uint8), 1)


def test_load_ema_keeps_the_tensors_pending_until_the_arena_exists():
    model = nn.Linear(3, 2)
    opt = _opt(ema_decay=0.9)
    state = {"decay": 0.9, "warmup": False, "updates": 5, "shadow": {"weight": torch.full((2, 3), 7.0)}}
    opt.load_ema(state, model)
    assert opt.ema_updates == 5 and opt.ema_buffers() is None          # no arena: still pending
    assert torch.equal(opt._ema_carry[id(model.weight)], torch.full((2, 3), 7.0))
    with pytest.raises(KeyError):
        opt.load_ema({"updates": 0, "shadow": {"nope": torch.zeros(1)}}, model)
    with pytest.raises(RuntimeError, match="shape"):
        opt.load_ema({"updates": 0, "shadow": {"bias": torch.zeros(3)}}, model)
    assert math.isclose(opt.ema_weight(), 0.1, rel_tol=1e-6)
