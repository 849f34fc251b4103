"""CPU: the LAMB layer-wise trust ratio of the arena AdamW step (AdamW.trust_ratio) -- everything that needs no device: the three entry
points are declared, exported and bound as declared; bad arguments are rejected before the GPU is touched; `trust_ratio` is a plain
attribute (default off, not in param_groups / defaults / state_dict) that get_optimization sets from `args.lamb`; anything but a bool
raises when the step is taken; the two int32 tables; and `lamb_statement`, the numpy fp64 statement of the semantics that the GPU tests
(tests/test_lamb_gpu.py) compare the kernels with."""
import subprocess

import numpy as np
import pytest
import torch
from torch import nn

from test_abi import ctype_of, header_decls

NEW = {
    "ytvln_lamb_stage1": ["const float* p", "const void* g", "int g_dtype", "float* m", "float* v", "const void* chunks", "int nchunks",
                          "const float* hyper", "float grad_scale", "const float* clip", "float* partials", "void* stream"],
    "ytvln_lamb_trust": ["const float* partials", "const void* chunks", "const int32_t* tensor_first", "const int32_t* rec_tensor",
                         "int ntensors", "float* trust", "float* report", "const float* clip", "void* stream"],
    "ytvln_lamb_stage2": ["float* p", "const float* m", "const float* v", "uint16_t* p_bf16", "const void* chunks", "int nchunks",
                          "const float* hyper", "const float* trust", "const int32_t* rec_tensor", "const float* clip", "void* stream"],
}


def lamb_statement(p, g, m, v, tensors, hyper, gscale=1.0):
    """One LAMB step in fp64 over `tensors` = [(offset, numel, wd)] of flat arrays, `hyper` = the eight floats of a launch class
    (beta1, beta2, eps, lr * b, lr, b, -, -) taken at the values the device reads (float32), `gscale` = grad_scale (times the clip
    coefficient).  Returns (p, m, v: float64 copies with the tensors' ranges updated; rows: [||p||, ||r||, trust] per tensor;
    r: float64, the direction on the tensors' ranges).

        m = beta1 m + (1 - beta1) g;   v = beta2 v + (1 - beta2) g g;   r = b m / (sqrt(v) + eps) + wd p      (p: before the update)
        trust = ||p|| / ||r|| if wd != 0 and both norms are finite and > 0 else 1;   p = p - lr trust r"""
    h = np.asarray(hyper, dtype=np.float32).astype(np.float64)
    b1, b2, eps, lr, b = h[0], h[1], h[2], h[4], h[5]
    p, m, v = (np.array(x, dtype=np.float64) for x in (p, m, v))
    g = np.asarray(g, dtype=np.float64) * float(gscale)
    r = np.zeros_like(p)
    rows = []
    for off, numel, wd in tensors:
        s = slice(off, off + numel)
        wd = float(np.float32(wd))
        m[s] = b1 * m[s] + (1.0 - b1) * g[s]
        v[s] = b2 * v[s] + (1.0 - b2) * g[s] * g[s]
        with np.errstate(all="ignore"):
            r[s] = b * m[s] / (np.sqrt(v[s]) + eps) + wd * p[s]
            np_, nr = float(np.sqrt(np.sum(p[s] * p[s]))), float(np.sqrt(np.sum(r[s] * r[s])))
        ok = wd != 0.0 and np.isfinite(np_) and np.isfinite(nr) and np_ > 0.0 and nr > 0.0
        trust = np_ / nr if ok else 1.0
        p[s] = p[s] - lr * trust * r[s]
        rows.append((np_, nr, trust))
    return p, m, v, np.array(rows, dtype=np.float64).reshape(-1, 3), r


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

    ok1 = dict(p=A, g=A, dt=_lib.DT_F32, m=A, v=A, ch=A, n=1, hy=A, gs=1.0, clip=None, part=B)

    def stage1(**kw):
        a = dict(ok1, **kw)
        return lib.ytvln_lamb_stage1(a["p"], a["g"], a["dt"], a["m"], a["v"], a["ch"], a["n"], a["hy"], a["gs"], a["clip"], a["part"], None)
    for k in ("p", "g", "m", "v", "ch", "hy", "part"):
        assert stage1(**{k: None}) != 0 and b"null" in err(), k
    for k in ("p", "g", "m", "v"):
        assert stage1(**{k: A + 8}) != 0 and b"aligned" in err(), k
    assert stage1(part=B + 4) != 0 and b"aligned" in err()
    for dt in (_lib.DT_F64, _lib.DT_I64, _lib.DT_U8, -1, 17):
        assert stage1(dt=dt) != 0 and b"dtype" in err()
    assert stage1(n=-1) != 0 and b"nchunks" in err()
    assert stage1(n=0) == 0 and stage1(n=0, dt=_lib.DT_BF16, clip=B) == 0          # empty table: no-op

    ok2 = dict(part=A, ch=A, first=A, rec=A, nt=1, trust=B, rep=B, clip=None)

    def trust(**kw):
        a = dict(ok2, **kw)
        return lib.ytvln_lamb_trust(a["part"], a["ch"], a["first"], a["rec"], a["nt"], a["trust"], a["rep"], a["clip"], None)
    for k in ("part", "ch", "first", "rec", "trust", "rep"):
        assert trust(**{k: None}) != 0 and b"null" in err(), k
    assert trust(part=A + 4) != 0 and b"aligned" in err()
    assert trust(rep=B + 8) != 0 and b"aligned" in err()
    assert trust(nt=-2) != 0 and b"ntensors" in err()
    assert trust(nt=0) == 0

    ok3 = dict(p=A, m=A, v=A, pb=None, ch=A, n=1, hy=A, trust=B, rec=B, clip=None)

    def stage2(**kw):
        a = dict(ok3, **kw)
        return lib.ytvln_lamb_stage2(a["p"], a["m"], a["v"], a["pb"], a["ch"], a["n"], a["hy"], a["trust"], a["rec"], a["clip"], None)
    for k in ("p", "m", "v", "ch", "hy", "trust", "rec"):
        assert stage2(**{k: None}) != 0 and b"null" in err(), k
    for k in ("p", "m", "v", "pb"):
        assert stage2(**{k: A + 8}) != 0 and b"aligned" in err(), k
    assert stage2(n=-1) != 0 and b"nchunks" in err()
    assert stage2(n=0) == 0 and stage2(n=0, pb=B, clip=B) == 0
    with pytest.raises(RuntimeError, match="ytvln_lamb_stage1 failed"):
        _lib.call("ytvln_lamb_stage1", A, A, _lib.DT_F64, A, A, A, 1, A, 1.0, None, B, None)


def _args(**kw):
    from helpers import args_ns
    return args_ns(**kw)


def test_get_optimization_sets_the_attribute_from_args_lamb():
    from ytvln.vilbert_init import get_optimization
    model = nn.Linear(4, 4)
    opt, _, _, _ = get_optimization(_args(), model, 10, None)          # an argument object without the field: off
    assert opt.trust_ratio is False and opt.lamb_setting() is False
    opt, _, _, _ = get_optimization(_args(lamb=True), model, 10, None)
    assert opt.trust_ratio is True and opt.lamb_setting() is True
    opt, _, _, _ = get_optimization(_args(lamb=False), model, 10, None)
    assert opt.trust_ratio is False
    assert opt.max_grad_norm is None and opt.skip_nonfinite is False          # the clip attributes are untouched by it


def test_attribute_is_not_a_constructor_argument_nor_optimizer_state():
    from ytvln.optimization import AdamW
    with pytest.raises(TypeError):
        AdamW([nn.Parameter(torch.zeros(4))], lr=1e-3, trust_ratio=True)
    ps = [nn.Parameter(torch.zeros(4)), nn.Parameter(torch.zeros(3))]
    plain = AdamW(ps, lr=1e-3)
    on = AdamW(ps, lr=1e-3)
    assert plain.trust_ratio is False
    on.trust_ratio = True
    sa, sb = plain.state_dict(), on.state_dict()
    assert sa.keys() == sb.keys() and sa["state"].keys() == sb["state"].keys()
    assert [sorted(g) for g in sa["param_groups"]] == [sorted(g) for g in sb["param_groups"]]
    assert repr(sa) == repr(sb)
    assert plain.defaults == on.defaults and "trust_ratio" not in on.defaults
    assert all("trust_ratio" not in g for g in on.param_groups)
    assert on.lamb_buffers() is None          # no arena yet: nothing to allocate
    with pytest.raises(RuntimeError, match="no step has been taken"):
        on.trust_ratios()


@pytest.mark.parametrize("bad", [1, 0, 1.0, "True", None, [True], torch.tensor(True), np.bool_(True)])
def test_anything_but_a_bool_raises_when_the_step_is_taken(bad):
    from ytvln.optimization import AdamW
    p = nn.Parameter(torch.zeros(4))
    opt = AdamW([p], lr=1e-3)
    opt.trust_ratio = bad          # plain attribute: assignment itself never raises
    p.grad = torch.ones(4)
    with pytest.raises(ValueError, match="trust_ratio"):
        opt.step()
    with pytest.raises(ValueError, match="trust_ratio"):
        opt.lamb_setting()


def test_prepare_replay_refuses_a_setting_changed_after_a_capture():
    """A captured step bakes the setting in: the host-side check needs no device."""
    from ytvln.optimization import AdamW, CaptureSettings
    opt = AdamW([nn.Parameter(torch.zeros(4))], lr=1e-3)
    opt._launch = []                      # (no launch classes: prepare_replay uploads nothing)
    opt.trust_ratio = True
    opt.prepare_replay()                  # nothing captured yet: any setting goes
    opt._captured = CaptureSettings(lamb=False)          # as a capture with the feature off leaves it
    with pytest.raises(RuntimeError, match="capture the step again"):
        opt.prepare_replay()
    opt.trust_ratio = False
    opt.prepare_replay()
    opt._captured = CaptureSettings(lamb=True)          # as a capture with it on leaves it
    with pytest.raises(RuntimeError, match="capture the step again"):
        opt.prepare_replay()
    opt.trust_ratio = True
    opt.prepare_replay()
    opt.trust_ratio = 1
    with pytest.raises(ValueError, match="trust_ratio"):
        opt.prepare_replay()


def test_int32_tables_of_a_hand_made_member_list():
    from ytvln.optimization import CHUNK, lamb_tables
    assert CHUNK == 16384
    # (arena index, numel): one record, one record with a tail, an exact chunk, two records, three records with a ragged last one
    first, rec = lamb_tables([(4, 1), (0, 5), (7, CHUNK), (2, CHUNK + 1), (9, 40000)])
    assert first == [0, 1, 2, 3, 5, 8]
    assert rec == [4, 0, 7, 2, 2, 9, 9, 9]
    assert lamb_tables([]) == ([0], [])
    assert lamb_tables([(3, 10), (1, 3)], chunk=4) == ([0, 3, 4], [3, 3, 3, 1])
    with pytest.raises(ValueError):
        lamb_tables([(0, 0)])
    with pytest.raises(ValueError):
        lamb_tables([(-1, 4)])


def test_fp64_statement_of_the_semantics():
    hyper = np.array([0.9, 0.999, 1e-6, 0.0, 1e-2, 0.0, 0, 0], dtype=np.float32)
    t = 3
    b = np.sqrt(1 - float(hyper[1]) ** t) / (1 - float(hyper[0]) ** t)
    hyper[5], hyper[3] = b, hyper[4] * b
    h = hyper.astype(np.float64)
    rng = np.random.default_rng(3)
    n = 24
    p, g, m, v = rng.standard_normal(n), rng.standard_normal(n), 0.1 * rng.standard_normal(n), 0.01 * rng.random(n)
    p[16:20] = 0.0
    tensors = [(0, 7, 0.01), (8, 5, 0.0), (16, 4, 0.01), (20, 4, 0.01)]
    p1, m1, v1, rows, r = lamb_statement(p, g, m, v, tensors, hyper, gscale=0.5)
    # tensor 0, written out by hand
    s = slice(0, 7)
    gs = 0.5 * g[s]
    mm = h[0] * m[s] + (1 - h[0]) * gs
    vv = h[1] * v[s] + (1 - h[1]) * gs * gs
    rr = h[5] * mm / (np.sqrt(vv) + h[2]) + float(np.float32(0.01)) * p[s]
    tr = np.linalg.norm(p[s]) / np.linalg.norm(rr)
    assert np.allclose(m1[s], mm, rtol=1e-15) and np.allclose(v1[s], vv, rtol=1e-15) and np.allclose(r[s], rr, rtol=1e-15)
    assert abs(rows[0, 2] - tr) <= 1e-15 * tr and tr != 1.0
    assert np.allclose(p1[s], p[s] - h[4] * tr * rr, rtol=1e-15)
    # wd == 0: excluded from layer adaptation; all-zero p: trust 1 (and the update is then plain Adam's direction times lr)
    assert rows[1, 2] == 1.0 and rows[1, 0] > 0 and rows[1, 1] > 0
    assert rows[2, 2] == 1.0 and rows[2, 0] == 0.0
    assert np.array_equal(p1[16:20], -h[4] * r[16:20])
    # elements outside the tensors (alignment padding) are untouched
    for a0, a1 in ((p, p1), (m, m1), (v, v1)):
        assert a1[7] == a0[7] and np.array_equal(a1[13:16], a0[13:16])
    # a non-finite norm: trust 1
    g2 = g.copy()
    g2[21] = np.inf
    rows2 = lamb_statement(p, g2, m, v, tensors, hyper)[3]
    assert rows2[3, 2] == 1.0 and not np.isfinite(rows2[3, 1])
    # the inputs are not modified
    assert p[0] != p1[0] and m[0] != m1[0]
