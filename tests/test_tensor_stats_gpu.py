"""GPU: per-tensor gradient / weight statistics of the arena AdamW step (AdamW.tensor_stats; ytvln_tensor_stats_stage1 ->
ytvln_tensor_stats_stage2).

Bars and where they come from:
  * counts: exact integers.
  * maxima: bit-equal to torch's fp32 maximum of |x| over the finite elements, times float32(grad_scale) for the gradient (one fp32 product
    on both sides): a maximum is one of its inputs, no rounding takes part.
  * norms, relative 1e-5 against an fp64 reference over the finite elements.  Stage 1 keeps the summation tree of ytvln_grad_sumsq: a record
    holds at most CHUNK = 16384 elements, a thread of the 256-thread workgroup adds at most 64 squares serially into one fp32 accumulator
    (each an fma: the square itself is not rounded; a non-finite element adds the square of 0, which changes nothing), then the fixed tree
    adds 8 levels (6 in the wave, 2 across the 4 waves): a chain of <= 72 roundings, plus the fp32 rounding of the partial's use -- <= 73 *
    2^-24 = 4.4e-6 on a sum of non-negative terms in the worst case, half that on its root.  Stage 2 sums the partials in fp64 (nothing at
    this scale) and rounds the norm once to fp32 (6e-8).  Together below 2.3e-6: the bar of tests/test_grad_clip_gpu.py, NORM_RTOL = 1e-5,
    applies unchanged.  A root-sum-square of the rows against grad_norm() compares two such numbers: twice the bar.
  * everything called bit-identical is compared on the bits."""
import copy
import math
import os
import struct
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT
from test_rccl_gpu import _batch, _build, _free_port

pytestmark = pytest.mark.gpu

CHUNK = 16384
NORM_RTOL = 1e-5
NAN, INF = float("nan"), float("inf")

# ---- kernel level: a hand-built arena and hand-built tables -----------------------------------------------------------------------------
SIZES = [1, 3, 5, CHUNK, CHUNK + 1, 40000, 65 * CHUNK + 1]          # CHUNK + 1: a second record of length 1; 40000: three records; the last: 66
OFFS = []
_o = 8
for _n in SIZES:
    OFFS.append(_o)
    _o = (_o + _n + 3) // 4 * 4 + 4          # 4-aligned slots, at least four padding elements between them
N = _o + 4
TABLES = [[5, 0, 3], [6, 2, 4, 1]]          # arena indices in table order: neither table follows the arena, rec_tensor is not monotone
BAD_G = {0: 1, 3: 1, 4: 1, 5: 1}            # arena index -> non-finite gradient elements injected below


def _bits(t):
    return t.contiguous().view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class Arena:
    """p and g with NaN in every padding element; the injections of the module docstring's cases."""

    def __init__(self, dev, all_nan=False):
        from ytvln.optimization import lamb_tables
        assert all(o % 4 == 0 for o in OFFS) and all(OFFS[i] + SIZES[i] < OFFS[i + 1] for i in range(len(SIZES) - 1))
        gen = torch.Generator().manual_seed(19)
        self.p = torch.full((N,), NAN)
        self.g = torch.full((N,), NAN)
        for o, n in zip(OFFS, SIZES):
            self.p[o:o + n] = torch.randn(n, generator=gen)
            self.g[o:o + n] = torch.randn(n, generator=gen) * torch.exp2(torch.randint(-6, 6, (n,), generator=gen).float())
        self.g[OFFS[0]] = NAN                                  # the only element of the 1-element tensor: norm 0, max 0, count 1
        self.g[OFFS[4] + CHUNK] = NAN                          # the length-1 tail record
        self.g[OFFS[3] + CHUNK - 1] = INF                      # the last element of the 16384 tensor
        self.g[OFFS[5] + 2 * CHUNK + 100] = -INF               # inside the third record of the 40000 tensor
        self.p[OFFS[1] + 1] = INF                              # a non-finite parameter of the 3-element tensor
        self.bad_g = dict(BAD_G)
        if all_nan:
            self.g[OFFS[5]:OFFS[5] + SIZES[5]] = NAN
            self.bad_g[5] = SIZES[5]
        self.dev = dev
        self.tables = []
        rec0 = 0
        for order in TABLES:
            records = [(OFFS[k] + c, min(CHUNK, SIZES[k] - c)) for k in order for c in range(0, SIZES[k], CHUNK)]
            first, rec = lamb_tables([(k, SIZES[k]) for k in order])
            assert len(rec) == len(records) and any(rec[i] > rec[i + 1] for i in range(len(rec) - 1))
            table = torch.frombuffer(bytearray(b"".join(struct.pack("<qqff", o, n, 0.0, 0.0) for o, n in records)), dtype=torch.uint8).to(dev)
            self.tables.append(dict(table=table, n=len(records), rec0=rec0, first=torch.tensor(first, dtype=torch.int32, device=dev),
                                    rec=torch.tensor(rec, dtype=torch.int32, device=dev), nt=len(order)))
            rec0 += len(records)
        self.nrec = rec0
        assert self.nrec == 75 and max(t["n"] for t in self.tables) > 64

    def operands(self, dtype):
        """(p on the device, g on the device in `dtype`, the values the kernel sees as fp32 on the host)."""
        g = self.g.to(dtype)
        return self.p.to(self.dev), g.to(self.dev), g.float()

    def fresh_counts(self):
        counts = torch.zeros(len(SIZES) + 1, 3, dtype=torch.int64, device=self.dev)
        counts[-1] = 7
        return counts

    def launch(self, p, g, scale, counts):
        """Both stages over both tables; every output buffer carries spare slots that must stay untouched."""
        from ytvln import ops
        partials = torch.full((4 * self.nrec + 4,), 7.0, dtype=torch.float32, device=self.dev)
        bad = torch.full((2 * self.nrec + 2,), 7, dtype=torch.int32, device=self.dev)
        stats = torch.full((len(SIZES) + 1, 4), 7.0, dtype=torch.float32, device=self.dev)
        for t in self.tables:
            part, cnt = partials[4 * t["rec0"]:4 * (t["rec0"] + t["n"])], bad[2 * t["rec0"]:2 * (t["rec0"] + t["n"])]
            ops.tensor_stats_stage1(p, g, t["table"], t["n"], part, cnt)
            ops.tensor_stats_stage2(part, cnt, t["n"], t["first"], t["rec"], t["nt"], scale, stats, counts)
        torch.cuda.synchronize()
        assert bool((partials[-4:] == 7.0).all()) and bool((bad[-2:] == 7).all()) and bool((stats[-1] == 7.0).all())
        assert bool((counts[-1] == 7).all())
        return partials, bad, stats


def _expect(x, scale):
    """(count of non-finite elements, fp64 norm over the finite ones times scale, fp32 maximum of |x| over them times float32(scale))."""
    fin = torch.isfinite(x)
    xf = x[fin]
    norm = scale * math.sqrt(float((xf.double() ** 2).sum()))
    mx = xf.abs().max() if xf.numel() else torch.zeros((), dtype=torch.float32)
    return int((~fin).sum()), norm, mx * torch.tensor(scale, dtype=torch.float32)


@pytest.mark.parametrize("all_nan", [False, True], ids=["injections", "all-nan-tensor"])
@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_rows_of_a_hand_built_arena(dev, lib, dtype, scale, all_nan):
    A = Arena(dev, all_nan)
    p, g, gseen = A.operands(dtype)
    p0, g0 = p.clone(), g.clone()
    counts = A.fresh_counts()
    partials, bad, stats = A.launch(p, g, scale, counts)
    assert _same(p, p0) and _same(g, g0), "both arenas are read-only"
    st, ct = stats.cpu(), counts.cpu()
    worst = 0.0
    for k, (o, n) in enumerate(zip(OFFS, SIZES)):
        cg, ng, mg = _expect(gseen[o:o + n], scale)
        cp, np_, mp_ = _expect(A.p[o:o + n], 1.0)
        assert ct[k].tolist() == [cg, cp, 1 if cg else 0], (k, ct[k].tolist())
        assert cg == A.bad_g.get(k, 0) and cp == (1 if k == 1 else 0)
        assert _same(st[k, 1], mg) and _same(st[k, 3], mp_), (k, st[k].tolist(), float(mg), float(mp_))
        for got, want in ((float(st[k, 0]), ng), (float(st[k, 2]), np_)):
            if want == 0.0:
                assert got == 0.0, (k, got)
            else:
                worst = max(worst, abs(got - want) / want)
                assert abs(got - want) <= NORM_RTOL * want, (k, got, want)
    print(f"{dtype} scale {scale} all_nan {all_nan}: worst relative norm error {worst:.3e} (bar {NORM_RTOL:.0e})")
    assert st[0].tolist()[:2] == [0.0, 0.0], "an empty finite set gives norm 0 and maximum 0"
    if all_nan:
        assert st[5].tolist()[:2] == [0.0, 0.0] and ct[5, 0] == 40000
    # a second launch on the same inputs: the same bits, and the sticky count advances by exactly one per launch with a bad tensor
    before = counts.clone()
    partials2, bad2, stats2 = A.launch(p, g, scale, counts)
    assert _same(partials, partials2) and _same(bad, bad2) and _same(stats, stats2), "two launches must be bit-equal"
    assert torch.equal(counts[:, :2], before[:, :2])
    assert counts[:-1, 2].tolist() == [2 if k in A.bad_g else 0 for k in range(len(SIZES))]
    # a clean gradient afterwards: this step's counts return to 0, the sticky ones stay
    clean = torch.where(torch.isfinite(g.float()), g.float(), torch.ones((), device=dev)).to(dtype)
    A.launch(p, clean, scale, counts)
    assert counts[:-1, 0].tolist() == [0] * len(SIZES) and counts[:-1, 2].tolist() == [2 if k in A.bad_g else 0 for k in range(len(SIZES))]
    assert counts[1, 1] == 1


def test_empty_tables_and_bad_operands(dev, lib):
    from ytvln import ops
    A = Arena(dev)
    p, g, _ = A.operands(torch.float32)
    t = A.tables[0]
    partials = torch.full((4 * t["n"],), 3.0, device=dev)
    bad = torch.full((2 * t["n"],), 3, dtype=torch.int32, device=dev)
    stats = torch.full((len(SIZES), 4), 3.0, device=dev)
    counts = torch.full((len(SIZES), 3), 3, dtype=torch.int64, device=dev)
    ops.tensor_stats_stage1(p, g, t["table"], 0, partials, bad)                                   # no records: nothing is written
    ops.tensor_stats_stage2(partials, bad, 0, t["first"], t["rec"], 0, 1.0, stats, counts)      # no tensors: nothing is written
    torch.cuda.synchronize()
    assert bool((partials == 3.0).all()) and bool((bad == 3).all()) and bool((stats == 3.0).all()) and bool((counts == 3).all())
    with pytest.raises(RuntimeError, match="float32 or bfloat16"):
        ops.tensor_stats_stage1(p, g.half(), t["table"], t["n"], partials, bad)
    with pytest.raises(RuntimeError, match="four partials"):
        ops.tensor_stats_stage1(p, g, t["table"], t["n"], partials[:-4], bad)
    with pytest.raises(RuntimeError, match="must be"):
        ops.tensor_stats_stage2(partials, bad, t["n"], t["first"], t["rec"], t["nt"], 1.0, stats, counts.int())
    with pytest.raises(RuntimeError, match="three int64 per row"):
        ops.tensor_stats_stage2(partials, bad, t["n"], t["first"], t["rec"], t["nt"], 1.0, stats, counts[:-1])


# ---- optimizer level --------------------------------------------------------------------------------------------------------------------
def _optimizer(dev, **extra):
    from ytvln.vilbert_init import get_optimization
    model, args = _build(dev)
    args.learning_rate = 1e-3
    for k, v in extra.items():
        setattr(args, k, v)
    opt, sched, _, _ = get_optimization(args, model, 10, None)
    return model, args, opt, sched


def _three_steps(dev, stats, extra, bf16_operand):
    from ytvln import utils_init as U
    model, args, opt, sched = _optimizer(dev, tensor_stats=stats, **extra)
    if bf16_operand:          # the update reads the bf16 buffer the exchange hook packed, as behind a bf16 gradient exchange
        opt.exchange_dtype = torch.bfloat16
        opt.grad_sync = lambda flat, layout: opt.pack_grads()
    batch = _batch(dev)
    for i in range(3):
        U.train_step(model, opt, sched, batch, args, i, all_options=True)
        if i == 0:
            opt.bf16_arena()          # from here on the update launches refresh the bf16 weight copy
    torch.cuda.synchronize()
    return opt


@pytest.mark.parametrize("case", ["plain", "clip+skip", "lamb", "ema", "bf16-operand"])
def test_three_steps_are_bit_identical_with_the_attribute_on_and_off(dev, lib, case):
    extra = {"plain": {}, "clip+skip": {"max_grad_norm": 1.0, "skip_nonfinite_grads": True}, "lamb": {"lamb": True}, "ema": {"ema_decay": 0.9},
             "bf16-operand": {}}[case]
    off = _three_steps(dev, False, extra, case == "bf16-operand")
    on = _three_steps(dev, True, extra, case == "bf16-operand")
    assert off._arena["stats"] is None, "feature off: nothing may be allocated"
    assert on._arena["stats"] is not None
    keys = ["p", "m", "v", "pb"] + (["ema"] if case == "ema" else []) + (["gb"] if case == "bf16-operand" else [])
    for k in keys:
        assert on._arena[k] is not None and _same(on._arena[k], off._arena[k]), k
    stats, counts = on.tensor_stats_report()
    assert stats.shape == (len(on.arena_layout()), 4) and counts.shape == (len(on.arena_layout()), 3)
    assert bool((stats[:, 2] > 0).any()) and bool((counts == 0).all())
    with pytest.raises(RuntimeError, match="no step has been taken"):
        off.tensor_stats_report()


def _rows64(opt, g):
    """fp64 rows from the arenas read back: `g` is the gradient arena the update read, p is read now (after the step)."""
    rows = []
    for o, n in opt.arena_layout().values():
        gs, ps = g[o:o + n].float().cpu(), opt._arena["p"][o:o + n].cpu()
        rows.append((math.sqrt(float((gs.double() ** 2).sum())), gs.abs().max(), math.sqrt(float((ps.double() ** 2).sum())), ps.abs().max()))
    return rows


def test_rows_after_a_real_step_match_fp64_and_the_global_norm(dev, lib):
    from ytvln import utils_init as U
    model, args, opt, sched = _optimizer(dev, tensor_stats=True, max_grad_norm=INF)
    batch = _batch(dev)
    for i in range(2):
        U.train_step(model, opt, sched, batch, args, i, all_options=True)
    U.train_step(model, opt, None, batch, args, 2, all_options=True, optimizer_step=False)
    opt.step()
    torch.cuda.synchronize()
    assert opt.grad_scale == 1.0
    stats, counts = (t.cpu() for t in opt.tensor_stats_report())
    assert bool((counts == 0).all())
    rows = _rows64(opt, opt._arena["g"])          # the step adopted every gradient into the arena and the update does not write it
    worst = 0.0
    for k, (gn, gm, pn, pm) in enumerate(rows):
        for got, want in ((float(stats[k, 0]), gn), (float(stats[k, 2]), pn)):
            assert abs(got - want) <= NORM_RTOL * want, (k, got, want)
            worst = max(worst, abs(got - want) / want if want else 0.0)
        assert _same(stats[k, 1], gm) and _same(stats[k, 3], pm), k
    total, norm = math.sqrt(float((stats[:, 0].double() ** 2).sum())), float(opt.grad_norm())
    print(f"{len(rows)} rows: worst relative norm error {worst:.3e}; root-sum-square {total!r} vs grad_norm() {norm!r}")
    assert norm > 0 and abs(total - norm) <= 2 * NORM_RTOL * norm
    # the rows carry the names of the model's parameters, in arena order
    names, named = opt.tensor_names(model), dict(model.named_parameters())
    assert len(names) == len(rows) and len(set(names)) == len(names)
    assert [opt.arena_range(named[n]) for n in names] == list(opt.arena_layout().values())
    assert opt.nonfinite_tensors(model) == {}


def test_a_poisoned_gradient_is_localised(dev, lib):
    from ytvln import utils_init as U
    model, args, opt, sched = _optimizer(dev, tensor_stats=True, skip_nonfinite_grads=True)
    batch = _batch(dev)
    for i in range(2):
        _, metrics = U.train_step(model, opt, sched, batch, args, i, all_options=True)
        assert float(metrics["nonfinite_grad_tensors"]) == 0.0
    a = opt._arena
    lo, hi = a["g"].data_ptr(), a["g"].data_ptr() + 4 * a["g"].numel()
    for sticky in (1, 2):
        before = a["p"].clone()
        U.train_step(model, opt, None, batch, args, 2, all_options=True, optimizer_step=False)
        victim = next(p for p in model.parameters() if p.grad is not None and lo <= p.grad.data_ptr() < hi)
        o, n = opt.arena_range(victim)
        a["g"][o + n // 2] = NAN
        opt.step()
        sched.step()
        opt.zero_grad()
        assert opt.skipped_steps() == sticky and _same(a["p"], before), "a skipped step leaves the parameters bit-unchanged and still reports"
        row = list(opt.arena_layout()).index(id(victim))
        counts = opt.tensor_stats_report()[1].cpu()
        assert (counts[:, 0] > 0).nonzero().reshape(-1).tolist() == [row] and counts[row].tolist() == [1, 0, sticky]
        name = next(k for k, p in model.named_parameters() if p is victim)
        assert opt.nonfinite_tensors(model) == {name: (1, sticky)}
    # through train_step: a hook poisons one element of one parameter's gradient on its way into the arena
    pos = next(p for k, p in model.named_parameters() if k.endswith("embeddings.position_embeddings.weight"))
    assert opt.arena_range(pos) is not None and pos is not victim

    def poison(grad):
        grad = grad.clone()
        grad.view(-1)[3] = INF
        return grad
    handle = pos.register_hook(poison)
    _, metrics = U.train_step(model, opt, sched, batch, args, 4, all_options=True)
    handle.remove()
    assert float(metrics["nonfinite_grad_tensors"]) == 1.0 and opt.skipped_steps() == 3
    row = list(opt.arena_layout()).index(id(pos))
    assert opt.tensor_stats_report()[1][row].tolist() == [1, 0, 1]
    _, metrics = U.train_step(model, opt, sched, batch, args, 5, all_options=True)          # and training goes on
    assert float(metrics["nonfinite_grad_tensors"]) == 0.0 and opt.skipped_steps() == 3 and not _same(a["p"], before)
    # the key is absent with the attribute off
    model2, args2, opt2, sched2 = _optimizer(dev)
    _, metrics = U.train_step(model2, opt2, sched2, batch, args2, 0, all_options=True)
    assert "nonfinite_grad_tensors" not in metrics


def test_capture_and_two_replays_report_what_eager_steps_report(dev, lib):
    from ytvln import utils_init as U
    batches = [_batch(dev, seed=40 + i) for i in range(3)]
    finals = []
    for mode in ("eager", "graph"):
        model, args, opt, sched = _optimizer(dev, tensor_stats=True)
        U.train_step(model, opt, sched, batches[0], args, 0, all_options=True)
        if mode == "eager":
            for i in (1, 2):
                U.train_step(model, opt, sched, batches[i], args, i, all_options=True)
        else:
            static = [t.clone() for t in batches[1]]
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                U.train_step(model, opt, None, static, args, 0, all_options=True)
            for i in (1, 2):
                for s, t in zip(static, batches[i]):
                    s.copy_(t)
                opt.prepare_replay()
                g.replay()
                sched.step()
            opt.tensor_stats = False                                  # switched off after the capture: the next replay path refuses
            with pytest.raises(RuntimeError, match="capture the step again"):
                opt.prepare_replay()
            opt.tensor_stats = True
        torch.cuda.synchronize()
        finals.append([opt._arena["p"].clone()] + [t.clone() for t in opt.tensor_stats_report()])
    for x, y in zip(finals[0], finals[1]):
        assert _same(x, y)
    assert bool((finals[0][1][:, 0] > 0).any())
    # a capture before an eager step (or stats_buffers()) created the buffers is refused; a captured step with it off refuses switching on
    model, args, opt, sched = _optimizer(dev)
    U.train_step(model, opt, sched, batches[0], args, 0, all_options=True)
    U.train_step(model, opt, None, batches[0], args, 1, all_options=True, optimizer_step=False)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        opt.step()
    opt.tensor_stats = True
    with pytest.raises(RuntimeError, match="capture the step again"):
        opt.prepare_replay()
    assert opt._arena["stats"] is None
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        with pytest.raises(RuntimeError, match="take one eager step with it on"):
            opt.step()
    assert opt._arena["stats"] is None
    assert opt.stats_buffers() is not None          # eagerly: allocated, and a capture may follow


def test_load_state_dict_restarts_the_report_with_the_new_arena(dev, lib):
    from ytvln import utils_init as U
    model, args, opt, sched = _optimizer(dev, tensor_stats=True, skip_nonfinite_grads=True)
    batch = _batch(dev)
    U.train_step(model, opt, sched, batch, args, 0, all_options=True)
    U.train_step(model, opt, None, batch, args, 1, all_options=True, optimizer_step=False)
    a = opt._arena
    o, n = next(iter(opt.arena_layout().values()))
    opt._ensure_arena()
    a["g"][o] = INF
    opt.step()
    opt.zero_grad()
    assert int(opt.tensor_stats_report()[1][:, 2].sum()) == 1
    opt.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert opt._arena is None
    with pytest.raises(RuntimeError, match="no step has been taken"):
        opt.tensor_stats_report()
    U.train_step(model, opt, sched, batch, args, 2, all_options=True)
    stats, counts = opt.tensor_stats_report()
    assert opt._arena is not a and stats.shape == (len(opt.arena_layout()), 4) and counts.shape == (len(opt.arena_layout()), 3)
    assert bool((counts == 0).all()) and bool((stats[:, 2] > 0).any()), "the sticky counts restart with the arena"


# ---- GraphedTrainStep in a one-rank world -----------------------------------------------------------------------------------------------
def _graphed_worker(case, port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                          HSA_ENABLE_IPC_MODE_LEGACY="0")
        os.environ.pop("YTVLN_DP_GRAD_DTYPE", None)
        sys.path.insert(0, os.path.join(ROOT, "youtube-vln_amd"))
        import torch.distributed as dist
        from ytvln import distributed as D, utils_init as U
        from ytvln.vilbert_init import get_optimization
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(0)
        D.init_distributed(backend="gloo", force=True)
        mode, _, gdtype = case.partition("@")

        def run(kind, stats):
            model, args = _build(dev)
            args.learning_rate, args.tensor_stats = 1e-3, stats
            dp = D.DataParallel(model, bucket_bytes=64 << 10, collective="rccl", always_exchange=True, grad_dtype=gdtype or "fp32")
            opt, sched, _, _ = get_optimization(args, model, 10, None)
            dp.attach(opt)
            batch = _batch(dev)
            if kind == "eager":
                for i in range(3):
                    U.train_step(dp, opt, sched, batch, args, i, all_options=True)
            else:
                U.train_step(dp, opt, sched, batch, args, 0, all_options=True)
                fwd_bwd = lambda backward=None: U.train_step(dp, opt, None, batch, args, 0, all_options=True, optimizer_step=False,  # noqa: E731
                                                             backward=backward)[0]
                gs = D.GraphedTrainStep(dp, opt, fwd_bwd, bucket_bytes=64 << 10, mode=mode)
                assert gs.mode == mode and gs.exchange
                gs.step(sched)
                gs.step(sched)
            torch.cuda.synchronize()
            dp.comm.check_async_error()
            assert (opt.exchange_dtype == torch.bfloat16) == (gdtype == "bf16")
            out = dict(p=opt._arena["p"].cpu().numpy(), allocated=opt._arena["stats"] is not None)
            if stats:
                out["stats"], out["counts"] = (t.cpu().numpy() for t in opt.tensor_stats_report())
            dp.close()
            return out
        out = dict(eager=run("eager", True), on=run("graph", True), off=run("graph", False))
        dist.destroy_process_group()
        q.put(("ok", out))
    except Exception as e:      # surface the failure in the parent instead of a bare exit code
        import traceback
        q.put(("error", traceback.format_exc()))
        raise e


@pytest.mark.parametrize("case", ["phased", "split", "single", "phased@bf16"])
def test_graphed_step_in_a_one_rank_world_reports_what_the_eager_step_reports(dev, lib, case):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_graphed_worker, args=(case, _free_port(), q))
    p.start()
    status, out = q.get(timeout=600)
    p.join(timeout=120)
    assert status == "ok", out
    assert p.exitcode == 0
    eager, on, off = out["eager"], out["on"], out["off"]
    assert on["allocated"] and not off["allocated"]
    assert on["stats"].shape == eager["stats"].shape and on["stats"].shape[1] == 4 and (on["stats"][:, 0] > 0).any()
    assert on["stats"].tobytes() == eager["stats"].tobytes(), float(np.abs(on["stats"] - eager["stats"]).max())
    assert np.array_equal(on["counts"], eager["counts"]) and not on["counts"].any()
    assert on["p"].tobytes() == off["p"].tobytes() and on["p"].tobytes() == eager["p"].tobytes()
