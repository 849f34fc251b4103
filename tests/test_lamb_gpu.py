"""GPU: the LAMB layer-wise trust ratio of the arena AdamW step (AdamW.trust_ratio; ytvln_lamb_stage1 -> ytvln_lamb_trust ->
ytvln_lamb_stage2) against `lamb_statement`, the numpy fp64 statement of the semantics in tests/test_lamb_cpu.py.

Bars and where they come from (u = 2^-24, the unit roundoff of fp32; every hyper-parameter enters the statement at its float32 value):
  * m within 2 ulp of the statement: m' = fma(1 - b1, g, fl(m b1)); 1 - b1 is exact for b1 in [0.5, 1) (Sterbenz), so there are two roundings,
    fl(m b1) and the fma's: <= ulp(m b1) / 2 + ulp(m') / 2.  That is <= 1 ulp(m') when |m'| >= |m b1|, i.e. when g does not pull against m;
    with opposite signs the sum cancels and ulp(m') shrinks below the error already made in fl(m b1), whatever the kernel does.  So the
    2-ulp bar is asserted on data whose m has the sign of g (`aligned=True`), and on fully random m the bar is taken at the larger of
    |m'| and |m b1| (test_two_runs_give_identical_bits).
  * v within 2 ulp: v' = fma(fl((1 - b2) g), g, fl(v b2)), all terms >= 0: ulp(v b2) / 2 + u (1 - b2) g^2 + ulp(v') / 2 < 2 ulp(v').
  * trust, relative BOUND = 91 u = 5.4e-6.  A record holds at most CHUNK = 16384 elements: a thread adds at most 64 squares serially
    into one fp32 accumulator (fma: the square itself is not rounded), the fixed tree adds 8 levels (6 in the wave, 2 across the 4 waves)
    and the partial is rounded once more where it is stored: <= 73 u relative on a sum of non-negative terms, half of it on the root --
    73 u for the two norms of the ratio together; the partials are then summed in fp64.  r itself carries an element-wise error
    of <= 8 u relative to its larger term (m: 2 u, sqrt(v) from a v within 2 ulp: 2 u, the square root, the + eps, the division and
    the final fma one each), which enters ||r|| (8 u) and the update of every element (8 u); the ratio's and the product lr * trust's
    roundings to fp32 take the last 2.
  * p within BOUND * lr * trust * |r| + 2 ulp(p).
  * everything called bit-identical is compared with torch.equal on the bits."""
import os
import struct
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT
from test_lamb_cpu import lamb_statement
from test_rccl_gpu import _batch, _build, _flat, _free_port

pytestmark = pytest.mark.gpu

CHUNK = 16384
U24 = 2.0 ** -24
BOUND = 91 * U24
LENGTHS = [1, 3, 5, 1024, 16384, 16385, 40000]          # one record with / without a vector body, a tail of one element, an exact chunk, three records
WDS = [0.01, 0.0, 0.01, 0.0, 0.01, 0.0, 0.01]
CLASS_OF = [0, 1, 0, 0, 1, 0, 1]


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _hyper(lr, t, b1=0.9, b2=0.999, eps=1e-6):
    b = (1.0 - b2 ** t) ** 0.5 / (1.0 - b1 ** t)
    return np.array([b1, b2, eps, lr * b, lr, b, 0, 0], dtype=np.float32)


class Arena:
    """A hand-built arena: tensors a multiple of 4 elements apart, cut into CHUNK records, spread over launch classes with their own
    hyper-parameters; the int32 tables come from the optimizer's own builder."""

    def __init__(self, dev, lengths=LENGTHS, wds=WDS, class_of=CLASS_OF, hypers=None, seed=5, aligned=False):
        from ytvln.optimization import lamb_tables
        self.dev = dev
        offs, off = [], 0
        for n in lengths:
            offs.append(off)
            off += (n + 3) // 4 * 4
        self.n, self.offs, self.lengths, self.wds = off, offs, lengths, wds
        hypers = hypers or [_hyper(1e-3, 3), _hyper(5e-4, 7)]
        self.classes = []
        rec0 = 0
        for ci in sorted(set(class_of)):
            ks = [k for k in range(len(lengths)) if class_of[k] == ci]
            rec = b"".join(struct.pack("<qqff", offs[k] + c, min(CHUNK, lengths[k] - c), wds[k], 0.0)
                           for k in ks for c in range(0, lengths[k], CHUNK))
            first, rec_tensor = lamb_tables([(k, lengths[k]) for k in ks])
            n = len(rec) // 24
            assert n == len(rec_tensor) == first[-1]
            self.classes.append(dict(ks=ks, n=n, rec0=rec0, nt=len(ks), hyper_np=hypers[ci],
                                     table=torch.frombuffer(bytearray(rec), dtype=torch.uint8).to(dev),
                                     first=torch.tensor(first, dtype=torch.int32).to(dev), rec=torch.tensor(rec_tensor, dtype=torch.int32).to(dev),
                                     hyper=torch.from_numpy(hypers[ci]).to(dev), tensors=[(offs[k], lengths[k], wds[k]) for k in ks]))
            rec0 += n
        self.nrec = rec0
        rng = np.random.default_rng(seed)
        mask = np.zeros(off, dtype=bool)
        for o, n in zip(offs, lengths):
            mask[o:o + n] = True
        f = lambda x: np.where(mask, x, 0.0).astype(np.float32)          # noqa: E731  (the padding between tensors stays zero)
        self.p0, self.g0 = f(rng.standard_normal(off)), f(0.3 * rng.standard_normal(off))
        m = 0.1 * rng.standard_normal(off)
        self.m0 = f(np.copysign(m, self.g0) if aligned else m)
        self.v0 = f(0.01 * rng.random(off))

    def state(self, copy=False):
        s = {k: torch.from_numpy(getattr(self, k + "0")).to(self.dev) for k in "pmv"}
        s["partials"] = torch.full((2 * self.nrec,), 7.0, dtype=torch.float32, device=self.dev)
        s["trust"] = torch.full((len(self.lengths),), 7.0, dtype=torch.float32, device=self.dev)
        s["report"] = torch.full((len(self.lengths), 4), 7.0, dtype=torch.float32, device=self.dev)
        s["pb"] = torch.zeros(self.n, dtype=torch.bfloat16, device=self.dev) if copy else None
        return s

    def step(self, s, g, clip=None, gscale=1.0):
        from ytvln import ops
        for c in self.classes:
            part = s["partials"][2 * c["rec0"]:2 * (c["rec0"] + c["n"])]
            ops.lamb_stage1(s["p"], g, s["m"], s["v"], c["table"], c["n"], c["hyper"], part, gscale, clip)
            ops.lamb_trust(part, c["table"], c["n"], c["first"], c["rec"], c["nt"], s["trust"], s["report"], clip)
            ops.lamb_stage2(s["p"], s["m"], s["v"], c["table"], c["n"], c["hyper"], s["trust"], c["rec"], clip, p_bf16=s["pb"])
        torch.cuda.synchronize()


def _ulp(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def _compare(arena, before, s, g, what, strict_m=True, only=None):
    """The device state `s` against one statement step from `before` = (p, m, v) numpy float32 (`only`: these tensors)."""
    p0, m0, v0 = before
    got = {k: s[k].cpu().numpy().astype(np.float64) for k in "pmv"}
    trust, report = s["trust"].cpu().numpy().astype(np.float64), s["report"].cpu().numpy().astype(np.float64)
    for c in arena.classes:
        p1, m1, v1, rows, r = lamb_statement(p0, g, m0, v0, c["tensors"], c["hyper_np"])
        h = c["hyper_np"].astype(np.float64)
        for j, (k, (o, n, wd)) in enumerate(zip(c["ks"], c["tensors"])):
            if only is not None and k not in only:
                continue
            sl = slice(o, o + n)
            m_bar = 2 * _ulp(m1[sl]) if strict_m else 2 * _ulp(np.maximum(np.abs(m1[sl]), np.abs(h[0] * m0[sl].astype(np.float64))))
            em, ev = np.abs(got["m"][sl] - m1[sl]), np.abs(got["v"][sl] - v1[sl])
            np_, nr, tr = rows[j]
            et = abs(trust[k] - tr) / tr
            p_bar = BOUND * h[4] * tr * np.abs(r[sl]) + 2 * _ulp(p1[sl])
            ep = np.abs(got["p"][sl] - p1[sl])
            print(f"{what} tensor {k} (len {n}, wd {wd}): m {float((em / _ulp(m1[sl])).max()):.2f} ulp, v {float((ev / _ulp(v1[sl])).max()):.2f} ulp, "
                  f"trust {trust[k]!r} want {tr!r} rel {et:.2e} (bar {BOUND:.2e}), p worst err/bar {float((ep / p_bar).max()):.3f}")
            assert (em <= m_bar).all() and (ev <= 2 * _ulp(v1[sl])).all(), (what, k)
            assert et <= BOUND, (what, k, trust[k], tr)
            if wd == 0.0:
                assert trust[k] == 1.0, (what, k)
            assert abs(report[k, 0] - np_) <= BOUND * np_ and abs(report[k, 1] - nr) <= BOUND * nr, (what, k, report[k], np_, nr)
            assert report[k, 2] == trust[k] and report[k, 3] == 0.0
            assert (ep <= p_bar).all(), (what, k, float((ep / p_bar).max()))
    pad = np.ones(arena.n, dtype=bool)
    for o, n in zip(arena.offs, arena.lengths):
        pad[o:o + n] = False
    for k in "pmv":
        assert (got[k][pad] == 0.0).all(), "the padding between tensors must not be written"


# ---- kernel level -----------------------------------------------------------------------------------------------------------------------
def test_three_steps_match_the_fp64_statement(dev, lib):
    A = Arena(dev, aligned=True)
    s = A.state()
    g = torch.from_numpy(A.g0).to(dev)
    before = (A.p0, A.m0, A.v0)
    for step in range(3):
        A.step(s, g)
        _compare(A, before, s, A.g0, f"step {step}")
        before = tuple(s[k].cpu().numpy() for k in "pmv")          # the next step starts from the device's own state
    assert not torch.equal(s["p"].cpu(), torch.from_numpy(A.p0))
    assert (s["partials"] != 7.0).all()


def test_two_runs_give_identical_bits(dev, lib):
    A = Arena(dev, seed=6)                                          # m of either sign against g
    g = torch.from_numpy(A.g0).to(dev)
    runs = []
    for _ in range(2):
        s = A.state(copy=True)
        A.step(s, g)
        A.step(s, g)
        runs.append(s)
    for k in ("p", "m", "v", "trust", "report", "partials", "pb"):
        assert torch.equal(_bits(runs[0][k]), _bits(runs[1][k])), k
    s = A.state()
    A.step(s, g)
    _compare(A, (A.p0, A.m0, A.v0), s, A.g0, "random m", strict_m=False)


def test_excluded_and_degenerate_tensors_have_trust_one(dev, lib):
    """wd == 0; an all-zero p with wd != 0; a tensor whose r is all zero although p is not: with beta1 = 0.5, eps = 1, b = 1 and
    g = v = 0, m = -2 fl(wd p) gives m' = -fl(wd p), sqrt(v') + eps = 1 and r = fma(1, m', fl(wd p)) = 0 exactly."""
    lengths, wds = [40000, 16385, 5003, 3], [0.0, 0.01, 0.01, 0.01]
    hyper = np.array([0.5, 0.999, 1.0, 1e-3, 1e-3, 1.0, 0, 0], dtype=np.float32)
    A = Arena(dev, lengths, wds, [0, 0, 0, 0], [hyper], seed=8)
    o1, o2, o3 = A.offs[1], A.offs[2], A.offs[3]
    A.p0[o1:o1 + lengths[1]] = 0.0
    for o, n in ((o2, lengths[2]), (o3, lengths[3])):
        A.g0[o:o + n] = 0.0
        A.v0[o:o + n] = 0.0
        A.m0[o:o + n] = np.float32(-2.0) * (np.float32(0.01) * A.p0[o:o + n])
    s = A.state()
    A.step(s, torch.from_numpy(A.g0).to(dev))
    trust, report = s["trust"].cpu().numpy(), s["report"].cpu().numpy()
    print("trust", trust.tolist(), "report", report.tolist())
    assert trust.tolist() == [1.0, 1.0, 1.0, 1.0]
    assert report[0, 0] > 0 and report[0, 1] > 0                     # wd == 0: norms reported, ratio not applied
    assert report[1, 0] == 0.0 and report[1, 1] > 0                  # all-zero p
    assert report[2, 0] > 0 and report[2, 1] == 0.0 and report[3, 0] > 0 and report[3, 1] == 0.0          # r all zero
    p = s["p"].cpu().numpy()
    for o, n in ((o2, lengths[2]), (o3, lengths[3])):
        assert np.array_equal(p[o:o + n], A.p0[o:o + n]), "r == 0: the parameter must not move"
    # (the statement's fp64 r of the last two tensors is the rounding residue of fl(wd p), not 0: they are checked exactly above instead)
    _compare(A, (A.p0, A.m0, A.v0), s, A.g0, "degenerate", strict_m=False, only=(0, 1))


def test_bf16_copy_equals_the_rounded_parameter_on_every_element(dev, lib):
    A = Arena(dev, seed=9)
    s = A.state(copy=True)
    A.step(s, torch.from_numpy(A.g0).to(dev))
    assert torch.equal(_bits(s["pb"]), _bits(s["p"].to(torch.bfloat16)))
    assert bool((s["pb"] != 0).any())
    t = A.state()                                                      # and the copy changes nothing else
    A.step(t, torch.from_numpy(A.g0).to(dev))
    for k in ("p", "m", "v", "trust", "report"):
        assert torch.equal(_bits(s[k]), _bits(t[k])), k


def test_bf16_gradients_equal_the_fp32_form_on_the_widened_values(dev, lib):
    A = Arena(dev, seed=10)
    gb = torch.from_numpy(A.g0).to(dev).to(torch.bfloat16)
    a, b = A.state(copy=True), A.state(copy=True)
    for _ in range(2):
        A.step(a, gb, gscale=0.5)
        A.step(b, gb.float(), gscale=0.5)
    assert not torch.equal(gb.float().cpu(), torch.from_numpy(A.g0))
    for k in ("p", "m", "v", "trust", "report", "pb"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    assert not torch.equal(a["p"].cpu(), torch.from_numpy(A.p0))


def test_a_clip_coefficient_of_one_half_equals_halved_gradients(dev, lib):
    A = Arena(dev, seed=11)
    g = torch.from_numpy(A.g0).to(dev)
    clip = torch.tensor([123.0, 0.5, 0.0, 4.0], device=dev)
    a, b, c = A.state(copy=True), A.state(copy=True), A.state(copy=True)
    A.step(a, g, clip=clip)
    A.step(b, g * 0.5)                                                # halving is exact
    A.step(c, g)
    for k in ("p", "m", "v", "trust", "report", "pb"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    assert not torch.equal(a["p"], c["p"])
    assert clip.tolist() == [123.0, 0.5, 0.0, 4.0]                     # read-only for the three launches


@pytest.mark.parametrize("gdtype", [torch.float32, torch.bfloat16])
def test_a_skip_record_leaves_everything_untouched(dev, lib, gdtype):
    A = Arena(dev, seed=12)
    g = torch.from_numpy(A.g0).to(dev).to(gdtype)
    clip = torch.tensor([float("inf"), 0.0, 1.0, 3.0], device=dev)
    s, ref = A.state(copy=True), A.state(copy=True)
    s["pb"].fill_(0.5)
    ref["pb"].fill_(0.5)
    A.step(s, g, clip=clip)
    for k in ("p", "m", "v", "pb", "trust", "report", "partials"):
        assert torch.equal(_bits(s[k]), _bits(ref[k])), k
    clip[2] = 0.0                                                     # and the same launches do run without the flag
    clip[1] = 1.0
    A.step(s, g, clip=clip)
    assert not torch.equal(s["p"], ref["p"]) and (s["trust"] != 7.0).all()


def test_bad_arguments_return_an_error_with_a_message(dev, lib):
    from ytvln import _lib, ops
    A = Arena(dev)
    s = A.state()
    c = A.classes[0]
    g = torch.from_numpy(A.g0).to(dev)
    part = s["partials"][:2 * c["n"]]
    with pytest.raises(RuntimeError, match="float32 or bfloat16"):
        ops.lamb_stage1(s["p"], g.half(), s["m"], s["v"], c["table"], c["n"], c["hyper"], part)
    with pytest.raises(RuntimeError, match="g_dtype"):
        _lib.call("ytvln_lamb_stage1", s["p"].data_ptr(), g.data_ptr(), _lib.DT_F64, s["m"].data_ptr(), s["v"].data_ptr(),
                  c["table"].data_ptr(), c["n"], c["hyper"].data_ptr(), 1.0, None, part.data_ptr(), None)
    assert lib.ytvln_lamb_stage1(s["p"].data_ptr(), None, _lib.DT_F32, s["m"].data_ptr(), s["v"].data_ptr(), c["table"].data_ptr(), c["n"],
                                 c["hyper"].data_ptr(), 1.0, None, part.data_ptr(), None) != 0
    assert b"null" in lib.ytvln_last_error()
    assert lib.ytvln_lamb_stage2(s["p"].data_ptr(), s["m"].data_ptr(), s["v"].data_ptr(), None, c["table"].data_ptr(), -1, c["hyper"].data_ptr(),
                                 s["trust"].data_ptr(), c["rec"].data_ptr(), None, None) != 0
    assert b"nchunks" in lib.ytvln_last_error()
    assert lib.ytvln_lamb_trust(part.data_ptr(), c["table"].data_ptr(), c["first"].data_ptr(), c["rec"].data_ptr(), -1, s["trust"].data_ptr(),
                                s["report"].data_ptr(), None, None) != 0
    assert b"ntensors" in lib.ytvln_last_error()
    with pytest.raises(RuntimeError, match="room for"):
        ops.lamb_stage1(s["p"], g, s["m"], s["v"], c["table"], c["n"], c["hyper"], part[:2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lamb_stage1(s["p"].cpu(), g, s["m"], s["v"], c["table"], c["n"], c["hyper"], part)
    with pytest.raises(RuntimeError, match="int32"):
        ops.lamb_trust(part, c["table"], c["n"], c["first"].long(), c["rec"], c["nt"], s["trust"], s["report"])
    with pytest.raises(RuntimeError, match="int32"):
        ops.lamb_stage2(s["p"], s["m"], s["v"], c["table"], c["n"], c["hyper"], s["trust"], c["rec"][:1])
    torch.cuda.synchronize()
    for k, z in (("p", A.p0), ("m", A.m0), ("v", A.v0)):
        assert np.array_equal(s[k].cpu().numpy(), z), "a rejected call must not have launched anything"


# ---- optimizer level --------------------------------------------------------------------------------------------------------------------
def _optimizer(dev, lamb, **extra):
    from ytvln.vilbert_init import get_optimization
    model, args = _build(dev)
    args.learning_rate = 1e-3
    if lamb is not None:
        args.lamb = lamb
    for k, v in extra.items():
        setattr(args, k, v)
    opt, sched, _, _ = get_optimization(args, model, 10, None)
    return model, args, opt, sched


def _train(dev, steps, lamb, **extra):
    from ytvln import utils_init as U
    model, args, opt, sched = _optimizer(dev, lamb, **extra)
    batch = _batch(dev)
    for i in range(steps):
        U.train_step(model, opt, sched, batch, args, i, all_options=True)
    torch.cuda.synchronize()
    return model, opt


def test_default_off_is_the_plain_adamw_kernel_bit_for_bit(dev, lib):
    from ytvln import ops
    from ytvln import utils_init as U
    model, args, opt, sched = _optimizer(dev, None)
    assert opt.trust_ratio is False
    batch = _batch(dev)
    for i in range(2):
        U.train_step(model, opt, sched, batch, args, i, all_options=True)
    U.train_step(model, opt, None, batch, args, 2, all_options=True, optimizer_step=False)
    opt._ensure_arena()                                              # adopt the stray gradients now: step() then finds nothing left to copy
    a = opt._arena
    p, g, m, v = (a[k].clone() for k in "pgmv")
    p_before = p.clone()
    opt.step()
    for c in opt._launch:                                            # (the hyper-parameters of this step are still in the class's device buffer)
        ops.adamw_step(p, g, m, v, c["table"], c["n"], c["hyper"], opt.grad_scale)
    torch.cuda.synchronize()
    assert a["lamb"] is None, "feature off: nothing may be allocated"
    assert not torch.equal(p, p_before), "the step must have moved the parameters"
    for x, k in ((p, "p"), (m, "m"), (v, "v")):
        assert torch.equal(_bits(x), _bits(a[k])), k
    with pytest.raises(RuntimeError, match="no step has been taken"):
        opt.trust_ratios()


def test_three_eager_steps_with_the_trust_ratio_on(dev, lib):
    from ytvln.vilbert_init import NO_DECAY
    plain, _ = _train(dev, 3, False)
    model, opt = _train(dev, 3, True)
    a = opt._arena
    for k in "pmv":
        assert bool(torch.isfinite(a[k]).all()), k
    assert not np.array_equal(_flat(plain), _flat(model))
    rows = opt.trust_ratios()
    layout = opt.arena_layout()
    assert rows.is_cuda and tuple(rows.shape) == (len(layout), 4)
    rows = rows.cpu().numpy()
    names = {id(p): n for n, p in model.named_parameters()}
    assert np.isfinite(rows).all() and (rows[:, 3] == 0).all() and (rows[:, 2] > 0).all()
    adapted = 0
    for row, pid in zip(rows, layout):                                # arena order
        if any(tag in names[pid] for tag in NO_DECAY):
            assert row[2] == 1.0, names[pid]
        else:
            adapted += row[2] != 1.0
    print("trust ratios: min", float(rows[:, 2].min()), "max", float(rows[:, 2].max()), "adapted tensors", int(adapted), "of", len(layout))
    assert adapted > 0
    # a row is the pre-update norm of its tensor's slot in the arena: check one against the parameters of the step before
    before, _ = _train(dev, 2, True)
    pid, (o, n) = next((pid, rng) for pid, rng in layout.items() if not any(tag in names[pid] for tag in NO_DECAY))
    k = list(layout).index(pid)
    want = float(dict(before.named_parameters())[names[pid]].detach().double().norm())
    assert abs(float(rows[k, 0]) - want) <= BOUND * want, (names[pid], rows[k, 0], want)


def test_capture_and_two_replays_equal_three_eager_steps(dev, lib):
    from ytvln import utils_init as U
    finals = []
    for mode in ("eager", "graph"):
        model, args, opt, sched = _optimizer(dev, True)
        batch = _batch(dev)
        U.train_step(model, opt, sched, batch, args, 0, all_options=True)
        if mode == "eager":
            for i in range(1, 3):
                U.train_step(model, opt, sched, batch, args, i, all_options=True)
        else:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                U.train_step(model, opt, None, batch, args, 0, all_options=True)
            for i in range(1, 3):
                opt.prepare_replay()
                g.replay()
                sched.step()
            opt.trust_ratio = False                                   # changed after the capture: the next replay path refuses
            with pytest.raises(RuntimeError, match="capture the step again"):
                opt.prepare_replay()
            opt.trust_ratio = True
        torch.cuda.synchronize()
        a = opt._arena
        finals.append([a[k].clone() for k in "pmv"] + [opt.trust_ratios().clone()])
    for x, y in zip(finals[0], finals[1]):
        assert torch.equal(_bits(x), _bits(y)), float((x - y).abs().max())


def test_an_inf_gradient_with_clipping_and_skip_leaves_all_state_untouched(dev, lib):
    from ytvln import utils_init as U
    model, args, opt, sched = _optimizer(dev, True, max_grad_norm=1.0, skip_nonfinite_grads=True)
    batch = _batch(dev)
    for i in range(2):
        U.train_step(model, opt, sched, batch, args, i, all_options=True)
    assert opt.skipped_steps() == 0
    a = opt._arena
    before = [a[k].clone() for k in "pmv"] + [x.clone() for x in opt.lamb_buffers()[1:]]
    U.train_step(model, opt, None, batch, args, 2, all_options=True, optimizer_step=False)
    lo, hi = a["g"].data_ptr(), a["g"].data_ptr() + 4 * a["g"].numel()
    victim = next(p for p in model.parameters() if p.grad is not None and lo <= p.grad.data_ptr() < hi)
    o, n = opt.arena_range(victim)
    a["g"][o + n // 2] = float("inf")
    opt.step()
    sched.step()
    opt.zero_grad()
    assert opt.skipped_steps() == 1
    for old, new in zip(before, [a[k] for k in "pmv"] + list(opt.lamb_buffers()[1:])):
        assert torch.equal(_bits(old), _bits(new))
    U.train_step(model, opt, sched, batch, args, 3, all_options=True)          # and training goes on
    assert opt.skipped_steps() == 1 and not torch.equal(a["p"], before[0]) and bool(torch.isfinite(a["p"]).all())


def _exchange_worker(mode, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                          HSA_ENABLE_IPC_MODE_LEGACY="0")
        os.environ.pop("YTVLN_DP_GRAD_DTYPE", None)
        sys.path.insert(0, os.path.join(ROOT, "youtube-vln_amd"))
        import torch.distributed as dist
        from ytvln import distributed as D, ops, utils_init as U
        from ytvln.vilbert_init import get_optimization
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(0)
        D.init_distributed(backend="gloo", force=True)
        model, args = _build(dev)
        args.learning_rate, args.lamb = 1e-3, True
        dp = D.DataParallel(model, bucket_bytes=64 << 10, collective="rccl", always_exchange=True, grad_dtype="bf16")
        opt, sched, _, _ = get_optimization(args, model, 10, None)
        dp.attach(opt)
        batch = _batch(dev)
        if mode == "eager":
            for step in range(2):
                U.train_step(dp, opt, sched, batch, args, step, all_options=True)
            a = opt._arena
            p, m, v = (a[k].clone() for k in "pmv")
            U.train_step(dp, opt, sched, batch, args, 2, all_options=True)
        else:       # phased: every update is deferred to the end of the step and runs over the launch classes' own tables
            U.train_step(dp, opt, sched, batch, args, 0, all_options=True)
            fwd_bwd = lambda backward=None: U.train_step(dp, opt, None, batch, args, 0, all_options=True, optimizer_step=False,  # noqa: E731
                                                         backward=backward)[0]
            gs = D.GraphedTrainStep(dp, opt, fwd_bwd, bucket_bytes=64 << 10, mode="phased")
            assert gs.mode == "phased" and gs.exchange and len([g for g in gs._group_slices if g]) > 1
            gs.step(sched)
            torch.cuda.synchronize()
            a = opt._arena
            p, m, v = (a[k].clone() for k in "pmv")
            gs.step(sched)
        # the same step at kernel level: the bf16 sums the update read are still in the exchange buffer, the hyper-parameters in the classes
        gb = opt.grad_bf16()
        partials, trust, report = (torch.zeros_like(x) for x in opt.lamb_buffers())
        for c in opt._launch:
            part = partials[2 * c["rec0"]:2 * (c["rec0"] + c["n"])]
            ops.lamb_stage1(p, gb, m, v, c["table"], c["n"], c["hyper"], part, opt.grad_scale, None)
            ops.lamb_trust(part, c["table"], c["n"], c["tensor_first"], c["rec_tensor"], c["ntensors"], trust, report, None)
            ops.lamb_stage2(p, m, v, c["table"], c["n"], c["hyper"], trust, c["rec_tensor"], None)
        torch.cuda.synchronize()
        dp.comm.check_async_error()
        same = [bool(torch.equal(_bits(x), _bits(a[k]))) for x, k in ((p, "p"), (m, "m"), (v, "v"))]
        same.append(bool(torch.equal(_bits(report), _bits(opt.trust_ratios()))))
        out = dict(same=same, bf16=opt.exchange_dtype == torch.bfloat16, nonzero=bool((gb != 0).any()),
                   finite=bool(torch.isfinite(a["p"]).all()), adapted=int((opt.trust_ratios()[:, 2] != 1.0).sum()))
        dp.close()
        dist.destroy_process_group()
        q.put(("ok", out))
    except Exception as e:      # surface the failure in the parent instead of a bare exit code
        import traceback
        q.put(("error", traceback.format_exc()))
        raise e


@pytest.mark.parametrize("mode", ["eager", "phased"])
def test_one_rank_bf16_exchange_matches_the_kernel_level_bf16_form(dev, lib, mode):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_exchange_worker, args=(mode, _free_port(), q))
    p.start()
    status, out = q.get(timeout=600)
    p.join(timeout=120)
    assert status == "ok", out
    assert p.exitcode == 0
    print(out)
    assert out["bf16"] and out["nonzero"] and out["finite"] and out["adapted"] > 0
    assert out["same"] == [True, True, True, True]
