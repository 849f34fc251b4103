"""GPU: the EMA of the weights of the arena AdamW step (AdamW.ema_decay; ytvln_ema_update, ytvln_ema_swap).

Bars and where they come from (fp32: unit roundoff 2^-24):
  * one update, e' = fma(w, fl(p - e), e) against the fp64 statement e + w (p - e) at the fp32 value of w: the subtraction is rounded once
    (<= 2^-24 |p - e| <= 2^-23 max(|p|, |e|), then scaled by w < 1) and the fma once (<= 2^-24 |e'|, e' between e and p): together below
    2^-22 max(|p|, |e|) per element.
  * three optimizer steps against the fp64 recursion over parameter snapshots: three times that, 3 * 2^-22 ~ 7.2e-7 < 1e-6, times M, the
    largest |p| or |e| the element has seen (an error made in one step is carried into the next one scaled by 1 - w < 1).
  * everything called bit-identical is compared on the bits."""
import os
import struct
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT
from helpers import ZERO_DROP, args_ns, cfg_dict
from test_rccl_gpu import _batch, _build, _free_port

pytestmark = pytest.mark.gpu

CHUNK = 16384
N = 66000
# (offset, length): a full record; lengths 1, 3, 5; a tensor of 16387 elements cut into 16384 + 3; a record at an offset that is no multiple of
# 4 (scalar path); a record with a vector body AND a tail; a second full record; gaps between all of them and behind the last one
RECORDS = [(0, 16384), (16392, 1), (16400, 3), (16408, 5), (16420, 16384), (16420 + 16384, 3), (32813, 1029), (33848, 1031), (40000, 16384)]
SCALAR, BODY_TAIL = RECORDS[6], RECORDS[7]


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    if not a.is_floating_point():
        return a.dtype == b.dtype and torch.equal(a, b)
    return a.dtype == b.dtype and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


class Table:
    def __init__(self, dev, seed=3):
        assert all(o + n <= N for o, n in RECORDS) and all(RECORDS[i][0] + RECORDS[i][1] <= RECORDS[i + 1][0] for i in range(len(RECORDS) - 1))
        assert SCALAR[0] % 4 != 0 and all(o % 4 == 0 for o, _ in RECORDS if (o, _) != SCALAR)
        self.dev, self.n = dev, len(RECORDS)
        self.table = torch.frombuffer(bytearray(b"".join(struct.pack("<qqff", o, n, 0.0, 0.0) for o, n in RECORDS)), dtype=torch.uint8).to(dev)
        self.mask = np.zeros(N, dtype=bool)
        for o, n in RECORDS:
            self.mask[o:o + n] = True
        rng = np.random.default_rng(seed)
        self.p0 = rng.standard_normal(N).astype(np.float32)          # the sentinel pattern: random everywhere, gaps included
        self.e0 = (self.p0 + 0.1 * rng.standard_normal(N)).astype(np.float32)
        # the scalar-path record and the all-tail / body-and-tail records repeat (p, e) pairs that lie in the vector body of the first record
        for o, n in (SCALAR, BODY_TAIL, RECORDS[2]):
            self.p0[o:o + n], self.e0[o:o + n] = self.p0[:n], self.e0[:n]

    def state(self):
        return torch.from_numpy(self.p0).to(self.dev), torch.from_numpy(self.e0).to(self.dev)

    def hyper(self, w):
        return torch.tensor([0.9, 0.999, 1e-6, 1e-3, 1e-3, 1.0, w, 0.0], dtype=torch.float32, device=self.dev)


@pytest.fixture(scope="module")
def T(dev, lib):
    return Table(dev)


# ---- kernel level -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1e-4, 0.1, 0.5])
def test_update_matches_the_fp64_statement(T, w):
    from ytvln import ops
    p, e = T.state()
    ops.ema_update(p, e, T.table, T.n, T.hyper(w))
    torch.cuda.synchronize()
    w32 = float(np.float32(w))
    p64, e64 = T.p0.astype(np.float64), T.e0.astype(np.float64)
    want = e64 + w32 * (p64 - e64)
    got = e.cpu().numpy()
    err = np.abs(got.astype(np.float64) - want)[T.mask]
    bar = (2.0 ** -22 * np.maximum(np.abs(p64), np.abs(e64)))[T.mask]
    print(f"w = {w}: worst err / bar {float((err / bar).max()):.3f}")
    assert (err <= bar).all()
    assert np.array_equal(got[~T.mask].view(np.int32), T.e0[~T.mask].view(np.int32)), "elements outside the records must not be written"
    assert np.array_equal(p.cpu().numpy().view(np.int32), T.p0.view(np.int32)), "p is read-only"
    assert not np.array_equal(got[T.mask], T.e0[T.mask])


@pytest.mark.parametrize("w", [1e-4, 0.1, 0.5, 1.0 - 2.0 ** -24, 2.0 ** -126])
def test_a_shadow_equal_to_its_parameter_is_a_fixed_point(T, w):
    from ytvln import ops
    p, _ = T.state()
    e = p.clone()
    ops.ema_update(p, e, T.table, T.n, T.hyper(w))
    torch.cuda.synchronize()
    assert _same(e, p)


def test_vector_body_and_scalar_tail_round_alike(T):
    from ytvln import ops
    p, e = T.state()
    ops.ema_update(p, e, T.table, T.n, T.hyper(0.3))
    torch.cuda.synchronize()
    for o, n in (SCALAR, BODY_TAIL, RECORDS[2]):          # the same pairs on the scalar path / in a tail as in the first record's vector body
        assert not _same(e[o:o + n], torch.from_numpy(T.e0[o:o + n]).to(T.dev))
        assert _same(e[o:o + n], e[:n]), (o, n)


def test_a_skip_record_leaves_the_shadow_untouched(T):
    from ytvln import ops
    p, e = T.state()
    clip = torch.tensor([float("inf"), 0.0, 1.0, 3.0], device=T.dev)
    ops.ema_update(p, e, T.table, T.n, T.hyper(0.5), clip)
    torch.cuda.synchronize()
    assert _same(e, torch.from_numpy(T.e0).to(T.dev)) and clip.tolist() == [float("inf"), 0.0, 1.0, 3.0]
    clip = torch.tensor([2.0, 0.25, 0.0, 3.0], device=T.dev)          # not skipped: the coefficient is the update's business, not the EMA's
    ops.ema_update(p, e, T.table, T.n, T.hyper(0.5), clip)
    _, e2 = T.state()
    ops.ema_update(p, e2, T.table, T.n, T.hyper(0.5), None)
    torch.cuda.synchronize()
    assert _same(e, e2) and not _same(e, torch.from_numpy(T.e0).to(T.dev))


@pytest.mark.parametrize("copy", [False, True])
def test_swap_exchanges_bit_for_bit(T, copy):
    from ytvln import ops
    p, e = T.state()
    p0, e0 = p.clone(), e.clone()
    mask = torch.from_numpy(T.mask).to(T.dev)
    pb = torch.full((N,), 0.5, dtype=torch.bfloat16, device=T.dev) if copy else None
    ops.ema_swap(p, e, T.table, T.n, p_bf16=pb)
    torch.cuda.synchronize()
    assert _same(p[mask], e0[mask]) and _same(e[mask], p0[mask])
    assert _same(p[~mask], p0[~mask]) and _same(e[~mask], e0[~mask]), "gaps must not be touched"
    if copy:
        assert _same(pb[mask], p.to(torch.bfloat16)[mask]), "the bf16 copy is the rounding of the NEW p on every element of every record"
        assert bool((pb[~mask] == 0.5).all())
    ops.ema_swap(p, e, T.table, T.n, p_bf16=pb)
    torch.cuda.synchronize()
    assert _same(p, p0) and _same(e, e0), "two swaps are the identity"
    if copy:
        assert _same(pb[mask], p0.to(torch.bfloat16)[mask])


def test_a_rejected_call_leaves_all_buffers_unchanged(T, lib):
    from ytvln import ops
    p, e = T.state()
    pb = torch.full((N,), 0.5, dtype=torch.bfloat16, device=T.dev)
    hy = T.hyper(0.5)
    assert lib.ytvln_ema_update(p.data_ptr(), e.data_ptr(), T.table.data_ptr(), -1, hy.data_ptr(), None, None) < 0
    assert b"nchunks" in lib.ytvln_last_error()
    assert lib.ytvln_ema_update(p.data_ptr(), e.data_ptr() + 4, T.table.data_ptr(), T.n, hy.data_ptr(), None, None) < 0
    assert b"aligned" in lib.ytvln_last_error()
    assert lib.ytvln_ema_update(p.data_ptr(), e.data_ptr(), T.table.data_ptr(), T.n, None, None, None) < 0
    assert b"null" in lib.ytvln_last_error()
    assert lib.ytvln_ema_swap(p.data_ptr(), None, pb.data_ptr(), T.table.data_ptr(), T.n, None) < 0
    assert b"null" in lib.ytvln_last_error()
    assert lib.ytvln_ema_swap(p.data_ptr(), e.data_ptr(), pb.data_ptr() + 2, T.table.data_ptr(), T.n, None) < 0
    assert b"aligned" in lib.ytvln_last_error()
    with pytest.raises(RuntimeError, match="size of the parameter arena"):
        ops.ema_update(p, e[:-4], T.table, T.n, hy)
    with pytest.raises(RuntimeError, match="size of the parameter arena"):
        ops.ema_swap(p, e, T.table, T.n, p_bf16=pb[:-4])
    with pytest.raises(RuntimeError, match="must be"):
        ops.ema_swap(p, e.double(), T.table, T.n)
    with pytest.raises(RuntimeError, match="must be"):
        ops.ema_swap(p, e, T.table, T.n, p_bf16=pb.float())
    torch.cuda.synchronize()
    assert _same(p, torch.from_numpy(T.p0).to(T.dev)) and _same(e, torch.from_numpy(T.e0).to(T.dev)) and bool((pb == 0.5).all())


# ---- optimizer level --------------------------------------------------------------------------------------------------------------------
def _optimizer(dev, **extra):
    from ytvln.vilbert_init import get_optimization
    model, args = _build(dev)
    args.learning_rate = 1e-3
    for k, v in extra.items():
        setattr(args, k, v)
    opt, sched, _, _ = get_optimization(args, model, 10, None)
    return model, args, opt, sched


def _snapshot(model):
    return {n: p.detach().cpu().numpy().astype(np.float64) for n, p in model.named_parameters()}


@pytest.mark.parametrize("extra", [{}, {"ema_warmup": True}, {"lamb": True}, {"max_grad_norm": 1.0}], ids=["plain", "warmup", "lamb", "clip"])
def test_three_eager_steps_follow_the_fp64_recursion(dev, lib, extra):
    from ytvln import utils_init as U
    model, args, opt, sched = _optimizer(dev, ema_decay=0.9, **extra)
    assert opt.ema_decay == 0.9 and opt.ema_updates == 0
    batch = _batch(dev)
    snaps, ws = [_snapshot(model)], []
    for i in range(3):
        ws.append(opt.ema_weight())                                  # the fp32 weight this step uploads
        U.train_step(model, opt, sched, batch, args, i, all_options=True)
        torch.cuda.synchronize()
        snaps.append(_snapshot(model))
    d = [0.9, 0.9, 0.9] if "ema_warmup" not in extra else [min(0.9, (1 + n) / (10 + n)) for n in range(3)]
    assert ws == [float(np.float32(1.0 - x)) for x in d] and opt.ema_updates == 3
    shadow = opt.ema_parameters()
    names = {id(p): n for n, p in model.named_parameters()}
    no_grad = [n for n, p in model.named_parameters() if opt.arena_range(p) is None]          # never received a gradient: no shadow
    assert len(shadow) == len(opt.arena_layout()) and len(shadow) + len(no_grad) == len(names) and len(shadow) > 0
    assert all(names[id(p)] not in no_grad for p in shadow)
    worst, moved = 0.0, 0
    for p, view in shadow.items():
        n = names[id(p)]
        assert view.shape == p.shape and view.data_ptr() != p.data_ptr()
        e = snaps[0][n]
        M = np.abs(e)
        for k in range(3):
            e = e + ws[k] * (snaps[k + 1][n] - e)
            M = np.maximum(M, np.maximum(np.abs(snaps[k + 1][n]), np.abs(e)))
        err = np.abs(view.cpu().numpy().astype(np.float64) - e)
        assert (err <= 1e-6 * M).all(), (n, float((err / np.maximum(M, 1e-300)).max()))
        worst = max(worst, float((err / np.maximum(M, 1e-300)).max()))
        moved += not np.array_equal(e, snaps[3][n])
    print(f"{extra}: worst |shadow - recursion| / M = {worst:.3e} (bar 1e-6), {moved} of {len(shadow)} shadows differ from their weights")
    assert moved > 0
    if "max_grad_norm" in extra:
        print("clip record [norm, coef, skip, skipped]:", opt._arena["clip"].tolist())


def test_capture_and_two_replays_equal_three_eager_steps(dev, lib):
    from ytvln import utils_init as U
    finals = []
    for mode in ("eager", "graph"):
        model, args, opt, sched = _optimizer(dev, ema_decay=0.9)
        batch = _batch(dev)
        U.train_step(model, opt, sched, batch, args, 0, all_options=True)
        if mode == "eager":
            U.train_step(model, opt, sched, batch, args, 1, all_options=True)
            opt.ema_decay = 0.5
            U.train_step(model, opt, sched, batch, args, 2, all_options=True)
        else:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                U.train_step(model, opt, None, batch, args, 0, all_options=True)
            assert opt.ema_updates == 1, "a capture is not an update"
            opt.prepare_replay()
            g.replay()
            sched.step()
            opt.ema_decay = 0.5                                       # travels by value: no recapture
            opt.prepare_replay()
            g.replay()
            sched.step()
            opt.ema_decay = None                                      # switched off after the capture: the next replay path refuses
            with pytest.raises(RuntimeError, match="capture the step again"):
                opt.prepare_replay()
            opt.ema_decay = 0.5
        torch.cuda.synchronize()
        assert opt.ema_updates == 3
        finals.append([opt._arena[k].clone() for k in ("p", "m", "v", "ema")])
    for x, y in zip(finals[0], finals[1]):
        assert _same(x, y), float((x - y).abs().max())
    assert not _same(finals[0][0], finals[0][3])


def test_capture_with_the_feature_off_is_untouched_and_refuses_switching_on(dev, lib):
    """The "off" half: a captured step without the EMA replays to the bits of eager steps, allocates no shadow, and switching the feature
    on afterwards is refused by prepare_replay() -- and by a capture before an eager step created the shadow."""
    from ytvln import utils_init as U
    finals = []
    for mode in ("eager", "graph"):
        model, args, opt, sched = _optimizer(dev)
        batch = _batch(dev)
        U.train_step(model, opt, sched, batch, args, 0, all_options=True)
        if mode == "eager":
            U.train_step(model, opt, sched, batch, args, 1, all_options=True)
        else:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                U.train_step(model, opt, None, batch, args, 0, all_options=True)
            opt.prepare_replay()
            g.replay()
            sched.step()
            opt.ema_decay = 0.9
            with pytest.raises(RuntimeError, match="capture the step again"):
                opt.prepare_replay()
            opt.ema_decay = None
        torch.cuda.synchronize()
        assert opt._arena["ema"] is None and opt.ema_updates == 0 and opt.ema_parameters() == {}
        assert all(float(c["hyper"][6]) == 0.0 for c in opt._launch)
        finals.append([opt._arena[k].clone() for k in "pmv"])
    for x, y in zip(finals[0], finals[1]):
        assert _same(x, y)


def test_an_inf_gradient_with_skip_nonfinite_leaves_the_shadow_untouched(dev, lib):
    from ytvln import utils_init as U
    model, args, opt, sched = _optimizer(dev, ema_decay=0.9, skip_nonfinite_grads=True)
    batch = _batch(dev)
    for i in range(2):
        U.train_step(model, opt, sched, batch, args, i, all_options=True)
    assert opt.skipped_steps() == 0 and opt.ema_updates == 2
    a = opt._arena
    before = [a[k].clone() for k in ("p", "m", "v", "ema")]
    assert not _same(before[0], before[3])
    U.train_step(model, opt, None, batch, args, 2, all_options=True, optimizer_step=False)
    lo, hi = a["g"].data_ptr(), a["g"].data_ptr() + 4 * a["g"].numel()
    victim = next(p for p in model.parameters() if p.grad is not None and lo <= p.grad.data_ptr() < hi)
    o, n = opt.arena_range(victim)
    a["g"][o + n // 2] = float("inf")
    opt.step()
    sched.step()
    opt.zero_grad()
    assert opt.skipped_steps() == 1
    assert opt.ema_updates == 3, "the host count advances on a step the device skips"
    for old, k in zip(before, ("p", "m", "v", "ema")):
        assert _same(old, a[k]), k
    U.train_step(model, opt, sched, batch, args, 3, all_options=True)          # and training goes on
    assert opt.skipped_steps() == 1 and not _same(a["ema"], before[3]) and bool(torch.isfinite(a["ema"]).all())


def _phased_worker(port, q):
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
        model, args = _build(dev)
        args.learning_rate, args.ema_decay = 1e-3, 0.9
        dp = D.DataParallel(model, bucket_bytes=64 << 10, collective="rccl", always_exchange=True)
        opt, sched, _, _ = get_optimization(args, model, 10, None)
        dp.attach(opt)
        batch = _batch(dev)
        U.train_step(dp, opt, sched, batch, args, 0, all_options=True)
        fwd_bwd = lambda backward=None: U.train_step(dp, opt, None, batch, args, 0, all_options=True, optimizer_step=False,  # noqa: E731
                                                     backward=backward)[0]
        gs = D.GraphedTrainStep(dp, opt, fwd_bwd, bucket_bytes=64 << 10, mode="phased")
        assert gs.mode == "phased" and gs.exchange and len([g for g in gs._group_slices if g]) > 1
        gs.step(sched)
        gs.step(sched)
        torch.cuda.synchronize()
        dp.comm.check_async_error()
        out = dict(shadow={k: v.cpu().numpy() for k, v in opt.ema_state_dict(model).items()},
                   weights={k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}, updates=opt.ema_updates)
        dp.close()
        dist.destroy_process_group()
        q.put(("ok", out))
    except Exception as e:      # surface the failure in the parent instead of a bare exit code
        import traceback
        q.put(("error", traceback.format_exc()))
        raise e


def test_phased_graphed_step_in_a_one_rank_world_equals_the_eager_run(dev, lib):
    from ytvln import utils_init as U
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_phased_worker, args=(_free_port(), q))
    p.start()
    status, out = q.get(timeout=600)
    p.join(timeout=120)
    assert status == "ok", out
    assert p.exitcode == 0
    model, args, opt, sched = _optimizer(dev, ema_decay=0.9)
    batch = _batch(dev)
    for i in range(3):
        U.train_step(model, opt, sched, batch, args, i, all_options=True)
    torch.cuda.synchronize()
    ref = {k: v.cpu().numpy() for k, v in opt.ema_state_dict(model).items()}
    weights = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    assert out["updates"] == opt.ema_updates == 3 and list(out["shadow"]) == list(ref)
    differ = 0
    for k in ref:
        assert out["shadow"][k].tobytes() == ref[k].tobytes(), k
        assert out["weights"][k].tobytes() == weights[k].tobytes(), k
        differ += not np.array_equal(ref[k], weights[k])
    assert differ > 0


def _eval_forward(model, batch):
    from ytvln import utils_init as U
    model.eval()
    with torch.no_grad():
        out = model(*U.get_model_input(batch, True))
    model.train()
    assert isinstance(out, dict) and len(out) > 0
    return [out[k].clone() for k in sorted(out) if torch.is_tensor(out[k])]


def test_ema_weights_block_evaluates_the_shadow_and_restores_the_weights(dev, lib):
    from ytvln import utils_init as U
    model, args, opt, sched = _optimizer(dev, ema_decay=0.9)
    batch = _batch(dev)
    for i in range(2):
        U.train_step(model, opt, sched, batch, args, i, all_options=True)
    a = opt._arena
    before = [a["p"].clone(), a["ema"].clone()]
    sd = opt.ema_state_dict(model)
    assert list(sd) == list(model.state_dict())
    plain = _eval_forward(model, batch)
    with opt.ema_weights():
        inside = _eval_forward(model, batch)
        assert _same(a["p"], before[1]) and _same(a["ema"], before[0])
        for k, v in model.state_dict().items():
            assert _same(v, sd[k]), k                                 # the swapped-in model IS the shadow file
        with pytest.raises(RuntimeError, match="swap"):
            opt.step()
        with pytest.raises(RuntimeError, match="swap"):
            opt.prepare_replay()
    assert _same(a["p"], before[0]) and _same(a["ema"], before[1])
    other, _ = _build(dev)
    other.load_state_dict(sd)
    want = _eval_forward(other, batch)
    assert len(inside) == len(want) > 0
    for x, y in zip(inside, want):
        assert _same(x, y)
    assert any(not _same(x, y) for x, y in zip(inside, plain)), "the shadow weights must give another forward than the trained ones"
    U.train_step(model, opt, sched, batch, args, 2, all_options=True)          # and training goes on
    assert opt.ema_updates == 3


def test_ema_weights_block_on_the_bf16_resident_path(dev, lib):
    """configs/tiny_2_2_1.json (head dimension 64), 2 pairs, 16 tokens, 8 regions: the swap refreshes the bf16 weight copy in the same pass."""
    from ytvln import ops, synth
    from ytvln import utils_init as U
    from ytvln.lily import Lily
    from ytvln.vilbert import BertConfig
    from ytvln.vilbert_init import get_optimization

    def build():
        args = args_ns(ranking=True, traj_judge=True, masked_vision=True, masked_language=True, learning_rate=1e-3, ema_decay=0.9)
        cfg = BertConfig(**cfg_dict("tiny_2_2_1.json", **ZERO_DROP))
        cfg.args = args
        model = Lily(cfg, dropout_prob=0.0)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(shapes, 3).items()})
        return model.to(dev).train(), args, cfg
    ops.set_matmul_precision("bf16")
    try:
        model, args, cfg = build()
        nb = synth.make_batch(bs=1, K=2, T=16, frames=2, boxes=4, seed=9, ignore_rank_frac=0.0)
        batch = synth.to_torch(nb, dev)
        assert cfg.hidden_size // cfg.num_attention_heads == 64
        opt, sched, _, _ = get_optimization(args, model, 10, None)
        for i in range(2):
            U.train_step(model, opt, sched, batch, args, i, all_options=True)
        a = opt._arena
        assert a["pb"] is not None, "the bf16-resident path must have made its weight copy"
        mask = torch.zeros(a["p"].numel(), dtype=torch.bool, device=dev)
        for o, n in opt.arena_layout().values():
            mask[o:o + n] = True
        assert _same(opt.bf16_arena()[mask], a["p"].to(torch.bfloat16)[mask])
        before = [a["p"].clone(), a["ema"].clone()]
        sd = opt.ema_state_dict(model)
        with opt.ema_weights():
            assert _same(a["p"], before[1])
            assert _same(opt.bf16_arena()[mask], a["p"].to(torch.bfloat16)[mask]), "the bf16 copy follows the swap on every element"
            inside = _eval_forward(model, batch)
            with pytest.raises(RuntimeError, match="swap"):
                opt.step()
        assert _same(a["p"], before[0]) and _same(a["ema"], before[1])
        assert _same(opt.bf16_arena()[mask], a["p"].to(torch.bfloat16)[mask])
        plain = _eval_forward(model, batch)
        other, _, _ = build()
        other.load_state_dict(sd)
        want = _eval_forward(other, batch)
        assert len(inside) == len(want) > 0
        for x, y in zip(inside, want):
            assert _same(x, y)
        assert any(not _same(x, y) for x, y in zip(inside, plain))
    finally:
        ops.set_matmul_precision("fp32")


def test_checkpoint_round_trip(dev, lib, tmp_path):
    from ytvln import utils_init as U
    from ytvln.vilbert_init import restore_checkpoint
    model, args, opt, sched = _optimizer(dev, ema_decay=0.9, ema_warmup=True)
    batch = _batch(dev)
    for i in range(2):
        U.train_step(model, opt, sched, batch, args, i, all_options=True)
    U.save_model(str(tmp_path), "on", None, model, opt, sched, 0)
    ckpt = torch.load(U.get_model_path(str(tmp_path), "on"), map_location="cpu")
    assert set(ckpt) == {"model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "epoch", "ytvln_rng_state", "ytvln_ema_state"}
    st = ckpt["ytvln_ema_state"]
    assert set(st) == {"decay", "warmup", "updates", "shadow"} and (st["decay"], st["warmup"], st["updates"]) == (0.9, True, 2)
    # every name of the model file whose tensor is an arena member (a tied weight appears under both of its names, as in state_dict())
    members = {k for k, v in model.state_dict(keep_vars=True).items() if opt.arena_range(v) is not None}
    assert set(st["shadow"]) == members and len(members) >= len(opt.ema_parameters()) > 0
    for k, v in opt.ema_state_dict(model).items():
        if k in members:
            assert _same(st["shadow"][k], v.cpu()), k
    model2, args2, opt2, sched2 = _optimizer(dev, ema_decay=0.9, ema_warmup=True)
    assert restore_checkpoint(U.get_model_path(str(tmp_path), "on"), model2, opt2, sched2) == 1
    assert opt2.ema_updates == 2 and opt2.ema_buffers() is None          # pending until the arena exists
    U.train_step(model, opt, sched, batch, args, 2, all_options=True)
    U.train_step(model2, opt2, sched2, batch, args2, 2, all_options=True)
    torch.cuda.synchronize()
    assert opt.ema_updates == opt2.ema_updates == 3
    sa, sb = opt.ema_state_dict(model), opt2.ema_state_dict(model2)
    assert list(sa) == list(sb)
    print("resumed against uninterrupted run: largest |difference| of a weight",
          max(float((x.double() - y.double()).abs().max()) for x, y in zip(model.state_dict().values(), model2.state_dict().values())),
          "of a shadow value", max(float((sa[k].double() - sb[k].double()).abs().max()) for k in sa))
    for k in sa:
        assert _same(sa[k], sb[k]), k
    for (k, x), (_, y) in zip(model.state_dict().items(), model2.state_dict().items()):
        assert _same(x, y), k
    assert not _same(opt._arena["ema"], opt._arena["p"])
    # feature off: exactly today's keys
    model3, args3, opt3, sched3 = _optimizer(dev)
    U.train_step(model3, opt3, sched3, batch, args3, 0, all_options=True)
    U.save_model(str(tmp_path), "off", None, model3, opt3, sched3, 0)
    off = torch.load(U.get_model_path(str(tmp_path), "off"), map_location="cpu")
    assert set(off) == {"model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "epoch", "ytvln_rng_state"}
    assert opt3._arena["ema"] is None


def test_optimizer_load_state_dict_mid_run_keeps_the_shadow(dev, lib):
    import copy
    from ytvln import utils_init as U
    model, args, opt, sched = _optimizer(dev, ema_decay=0.9)
    batch = _batch(dev)
    for i in range(2):
        U.train_step(model, opt, sched, batch, args, i, all_options=True)
    shadow = {p: v.clone() for p, v in opt.ema_parameters().items()}
    old = opt._arena["ema"]
    opt.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert opt._arena is None
    U.train_step(model, opt, None, batch, args, 2, all_options=True, optimizer_step=False)
    opt._ensure_arena()                                              # the rebuild: the shadow moves into the new arena before any update
    new = opt.ema_parameters()
    assert opt._arena["ema"] is not old and set(new) == set(shadow)
    for p, v in new.items():
        assert _same(v, shadow[p])
    opt.step()
    torch.cuda.synchronize()
    assert opt.ema_updates == 3 and any(not _same(v, shadow[p]) for p, v in opt.ema_parameters().items())
