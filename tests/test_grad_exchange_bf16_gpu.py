"""GPU: the opt-in bf16 gradient exchange of the data-parallel path (DataParallel(grad_dtype="bf16") / YTVLN_DP_GRAD_DTYPE=bf16).

Semantics (DDP's bf16 compression hook): every rank accumulates fp32 gradients in the AdamW arena, rounds them once per optimizer step
to bf16 (round to nearest even) into a send buffer of the same offsets, the buffer is SUM-all-reduced in bf16, and the fused AdamW reads
the bf16 sums with grad_scale = 1/world.  Covered here:
  * the two kernels: ytvln_grad_pack_bf16 against torch's fp32 -> bf16 conversion (specials, ties, gaps in the table, untouched
    elements), ytvln_adamw_f32_gbf16 bit-identical to ytvln_adamw_f32 fed the widened gradients;
  * a one-rank world with always_exchange (the exchange really runs, it is the identity): every step form equals, bit for bit, a plain
    run whose gradient arena is rounded to bf16 in place before every update, and differs from the fp32 exchange; half the payload;
  * two gloo ranks sharing the GPU: replicas equal each other and a single-process emulation of the bf16 sum; mixed dtypes refuse at wrap
    time on both ranks.
Every data-parallel case runs in spawned processes (process-group and communicator state never leak into the other GPU tests)."""
import os
import struct
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT
from test_rccl_gpu import _batch, _build, _flat, _free_port

pytestmark = pytest.mark.gpu

CHUNK = 16384


def _table(records, dev, wd=0.0):
    rec = b"".join(struct.pack("<qqff", o, n, wd, 0.0) for o, n in records)
    return torch.frombuffer(bytearray(rec), dtype=torch.uint8).to(dev), len(records)


def _bits16(t):
    return t.view(torch.int16).cpu().numpy()


# ---- kernels ----------------------------------------------------------------------------------------------------------------------
def test_grad_pack_bf16_matches_torch_rounding(dev, lib):
    from ytvln import ops
    n = 3 * CHUNK + 16000
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-40, 40, n))).astype(np.float32)
    bits = x.view(np.uint32)
    hi = rng.integers(0, 1 << 16, 4096, dtype=np.uint32)
    specials = np.concatenate([
        np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000,           # +-0, +-inf
                  0x7FC00000, 0xFFC00001, 0x7F800001, 0xFFBFFFFF,           # NaNs (quiet, signalling, negative)
                  0x00000001, 0x807FFFFF, 0x00400000, 0x00008000,           # fp32 subnormals (incl. a tie at the bottom)
                  0x00018000, 0x7F7FFFFF, 0xFF7F8000, 0x7F7F7FFF,           # tie between subnormals, max float (rounds to inf), ties near it
                  0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001], dtype=np.uint32),
        (hi << 16) | 0x8000,                                                # exact halfway between two bf16 values, even and odd below
        (hi[:512] << 16) | 0x7FFF, (hi[512:1024] << 16) | 0x8001,          # just below / above a tie
        rng.integers(1, 1 << 23, 256, dtype=np.uint32) | (rng.integers(0, 2, 256, dtype=np.uint32) << 31),   # random subnormals
    ])
    # specials at the head of records, inside them and in their scalar tails
    for start in (0, CHUNK + 4, 2 * CHUNK + 4000, n - len(specials)):
        bits[start:start + len(specials)] = specials
    g = torch.from_numpy(x.copy()).to(dev)
    # AdamW-like records (offsets multiples of 4, lengths <= CHUNK, odd ones, gaps between them) plus one misaligned record
    records = [(0, CHUNK), (CHUNK + 4, 1001), (CHUNK + 1012, 7), (CHUNK + 1024, 3), (CHUNK + 2000, CHUNK),
               (2 * CHUNK + 4000, CHUNK - 1), (n - len(specials) - 8, len(specials) + 7), (2 * CHUNK + 2001, 13)]
    covered = np.zeros(n, bool)
    for o, l in records:
        assert 0 <= o and o + l <= n and not covered[o:o + l].any()
        covered[o:o + l] = True
    table, nrec = _table(records, dev)
    sentinel = 0x5A5A
    gb = torch.full((n,), sentinel, dtype=torch.int16, device=dev).view(torch.bfloat16)
    ops.grad_pack_bf16(g, gb, table, nrec)
    torch.cuda.synchronize()
    got = _bits16(gb)
    want = _bits16(g.to(torch.bfloat16))
    assert (got[~covered] == sentinel).all(), "elements outside the chunk table were written"
    nan = np.isnan(x)
    assert nan[covered].sum() >= 4
    assert np.isnan(gb.float().cpu().numpy()[covered & nan]).all()
    ok = covered & ~nan
    bad = np.nonzero(got[ok] != want[ok])[0]
    assert bad.size == 0, [(hex(int(x.view(np.uint32)[ok][i])), hex(int(got[ok][i]) & 0xFFFF), hex(int(want[ok][i]) & 0xFFFF)) for i in bad[:8]]


@pytest.mark.parametrize("bf16copy", [False, True])
@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adamw_on_bf16_gradients_equals_fp32_kernel_on_widened_values(dev, lib, bf16copy, scale, wd):
    from ytvln import ops
    n = 2 * CHUNK + 5003
    gen = torch.Generator().manual_seed(11)
    p0 = torch.randn(n, generator=gen).to(dev)
    m0 = (0.1 * torch.randn(n, generator=gen)).to(dev)
    v0 = (0.01 * torch.rand(n, generator=gen)).to(dev)
    gb = (torch.randn(n, generator=gen) * 3).to(torch.bfloat16).to(dev)
    records = [(0, CHUNK), (CHUNK, CHUNK), (2 * CHUNK + 4, 4999)]      # element 2*CHUNK .. +3 not in the table: left alone by both
    table, nrec = _table(records, dev, wd)
    hyper = torch.tensor([0.9, 0.999, 1e-6, 1e-3 * (1 - 0.999 ** 3) ** 0.5 / (1 - 0.9 ** 3), 1e-3, 0, 0, 0], dtype=torch.float32, device=dev)
    outs = []
    for form in ("f32", "gbf16"):
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        pb = torch.zeros(n, dtype=torch.bfloat16, device=dev) if bf16copy else None
        for _ in range(2):
            if form == "f32":
                ops.adamw_step(p, gb.float(), m, v, table, nrec, hyper, scale, p_bf16=pb)
            else:
                ops.adamw_step_gbf16(p, gb, m, v, table, nrec, hyper, scale, p_bf16=pb)
        torch.cuda.synchronize()
        outs.append((p, m, v, pb))
    (p1, m1, v1, pb1), (p2, m2, v2, pb2) = outs
    assert not torch.equal(p1, p0)
    for a, b in ((p1, p2), (m1, m2), (v1, v2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    if bf16copy:
        assert torch.equal(pb1.view(torch.int16), pb2.view(torch.int16))
        inside = torch.ones(n, dtype=torch.bool, device=dev)
        inside[2 * CHUNK:2 * CHUNK + 4] = False                         # not in the table: the copy is not written there
        assert torch.equal(pb2[inside], p2[inside].to(torch.bfloat16)) and not pb2[~inside].any()


# ---- one-rank world, the exchange running ------------------------------------------------------------------------------------------
def _fwd_bwd(U, dp, opt, batch, args):
    return lambda backward=None: U.train_step(dp, opt, None, batch, args, 0, all_options=True, optimizer_step=False, backward=backward)[0]


def _one_rank_worker(case, port, q):
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
        case, _, precision = case.partition("@")
        ops.set_matmul_precision(precision or "fp32")
        collective, mode = case.split(":")
        mode, _, via = mode.partition("$")
        D.init_distributed(backend="nccl" if collective == "torch" else "gloo", force=True)
        out = {}
        for dtype in ("fp32", "bf16"):
            kw = {}
            if via == "env":
                os.environ["YTVLN_DP_GRAD_DTYPE"] = dtype
            else:
                kw["grad_dtype"] = dtype
            model, args = _build(dev, wide=bool(precision))
            args.learning_rate = 1e-3
            dp = D.DataParallel(model, bucket_bytes=64 << 10, collective=collective, always_exchange=True, **kw)
            assert dp.grad_dtype == {"fp32": torch.float32, "bf16": torch.bfloat16}[dtype]
            opt, sched, _, _ = get_optimization(args, model, 10, None)
            dp.attach(opt)
            batch = _batch(dev)
            digest = None
            if mode == "eager":
                for step in range(3):
                    U.train_step(dp, opt, sched, batch, args, step, all_options=True)
                assert dp._reducer.collectives == 3 * len(dp._reducer.buckets) and len(dp._reducer.buckets) > 1
                nbytes = dp.exchange_bytes_per_step()
            else:
                U.train_step(dp, opt, sched, batch, args, 0, all_options=True)
                gs = D.GraphedTrainStep(dp, opt, _fwd_bwd(U, dp, opt, batch, args), bucket_bytes=64 << 10, mode=mode)
                assert gs.mode == mode and gs.exchange and gs.grad_dtype == dp.grad_dtype
                for _ in range(2):
                    loss = gs.step(sched)
                assert torch.isfinite(loss).item()
                nbytes = gs.exchange_bytes_per_step()
                digest = gs.layout_digest()
            torch.cuda.synchronize()
            if dp.comm is not None:
                dp.comm.check_async_error()
            assert (opt._arena["gb"] is not None) == (dtype == "bf16"), "the bf16 buffer exists exactly when the bf16 exchange is in use"
            out[dtype] = (_flat(model), nbytes, digest)
            dp.close()
        os.environ.pop("YTVLN_DP_GRAD_DTYPE", None)
        dist.destroy_process_group()
        q.put(("ok", out))
    except Exception as e:      # surface the failure in the parent instead of a bare exit code
        import traceback
        q.put(("error", traceback.format_exc()))
        raise e


def _plain_rounded_run(dev, precision, steps=3):
    """The plain single-process run with the gradient arena rounded to bf16 in place before every update (grad_scale 1)."""
    from ytvln import ops, utils_init as U
    from ytvln.vilbert_init import get_optimization
    ops.set_matmul_precision(precision)
    try:
        model, args = _build(dev, wide=precision != "fp32")
        args.learning_rate = 1e-3
        opt, sched, _, _ = get_optimization(args, model, 10, None)
        opt.grad_sync = lambda flat, layout: flat.copy_(flat.bfloat16().float())
        batch = _batch(dev)
        for step in range(steps):
            U.train_step(model, opt, sched, batch, args, step, all_options=True)
        torch.cuda.synchronize()
        return _flat(model)
    finally:
        ops.set_matmul_precision("fp32")


@pytest.mark.parametrize("case", ["rccl:eager", "rccl:split", "rccl:single", "rccl:phased", "rccl:phased@bf16", "torch:eager", "torch:split",
                                  "rccl:eager$env", "rccl:phased$env"])
def test_one_rank_bf16_exchange_equals_rounded_plain_run(dev, lib, case):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_one_rank_worker, args=(case, _free_port(), q))
    p.start()
    status, out = q.get(timeout=900)
    p.join(timeout=120)
    assert status == "ok", out
    assert p.exitcode == 0
    precision = case.partition("@")[2] or "fp32"
    (w32, b32, d32), (w16, b16, d16) = out["fp32"], out["bf16"]
    ref = _plain_rounded_run(dev, precision)
    assert np.array_equal(w16, ref), float(np.abs(w16 - ref).max())
    assert not np.array_equal(w16, w32), "the bf16 exchange must round: it cannot equal the fp32 exchange"
    assert b32 > 0 and b16 * 2 == b32, (b16, b32)
    if not case.startswith(("rccl:eager", "torch:eager")):
        assert d16 != d32, "layout_digest must carry the exchange dtype"


# ---- two gloo ranks sharing the GPU ------------------------------------------------------------------------------------------------
def _two_rank_worker(rank, world, port, q, mode, dtypes):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                          HSA_ENABLE_IPC_MODE_LEGACY="0")
        os.environ.pop("YTVLN_DP_GRAD_DTYPE", None)
        sys.path.insert(0, os.path.join(ROOT, "youtube-vln_amd"))
        import torch.distributed as dist
        from ytvln import distributed as D, utils_init as U
        from ytvln.vilbert_init import get_optimization
        from test_dp_gpu import _batch as _rank_batch
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(0)
        D.init_distributed(backend="gloo")
        model, args = _build(dev)
        args.learning_rate = 1e-3
        try:
            dp = D.DataParallel(model, bucket_bytes=64 << 10, collective="torch", grad_dtype=dtypes[rank])
        except RuntimeError as e:
            dist.destroy_process_group()
            q.put((rank, "refused", str(e)))
            return
        if mode == "mixed":
            q.put((rank, "accepted", None))
            return
        opt, sched, _, _ = get_optimization(args, model, 10, None)
        dp.attach(opt)
        assert opt.grad_scale == 0.5 and opt.exchange_dtype == torch.bfloat16
        batch = _rank_batch(rank, dev)
        if mode == "accum":
            args.gradient_accumulation_steps = 2
            batch2 = _rank_batch(rank + 2, dev)
            for step in range(6):
                U.train_step(dp, opt, sched, batch if step % 2 == 0 else batch2, args, step, all_options=True)
        elif mode == "eager":
            for step in range(3):
                U.train_step(dp, opt, sched, batch, args, step, all_options=True)
        else:
            U.train_step(dp, opt, sched, batch, args, 0, all_options=True)
            if mode == "phased":
                os.environ["YTVLN_DP_CUTS"] = "t0,c0,v1"
            gs = D.GraphedTrainStep(dp, opt, _fwd_bwd(U, dp, opt, batch, args), bucket_bytes=64 << 10,
                                    mode="phased" if mode == "phased" else None)
            assert gs.mode == ("phased" if mode == "phased" else "split") and gs.grad_dtype == torch.bfloat16
            gs.verify_layout_across_ranks()
            for _ in range(2):
                loss = gs.step(sched)
            assert torch.isfinite(loss).item()
        torch.cuda.synchronize()
        flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu()
        both = [torch.zeros_like(flat) for _ in range(world)]
        dist.all_gather(both, flat)
        assert torch.equal(both[0], both[1]), "replicas diverged"
        dist.destroy_process_group()
        q.put((rank, "ok", flat.numpy() if rank == 0 else None))
    except Exception as e:
        import traceback
        q.put((rank, "error", traceback.format_exc()))
        raise e


def _emulate_two_ranks(dev, mode):
    """Single process: each rank's fp32 gradients from its own replica, summed as bf16(float(bf16(g0)) + float(bf16(g1))), then the fp32
    AdamW on the widened sums with grad_scale 0.5 (bit-identical to the bf16-gradient kernel).  Rank 1's micro-steps run inside rank 0's
    exchange hook, when both replicas still hold the same weights."""
    from ytvln import utils_init as U
    from ytvln.vilbert_init import get_optimization
    from test_dp_gpu import _batch as _rank_batch
    accum = 2 if mode == "accum" else 1
    reps = []
    for r in range(2):
        model, args = _build(dev)
        args.learning_rate = 1e-3
        opt, sched, _, _ = get_optimization(args, model, 10, None)
        args.gradient_accumulation_steps = accum          # after the schedule is built, as in the data-parallel run
        opt.grad_scale = 0.5
        batches = [_rank_batch(r, dev)] + ([_rank_batch(r + 2, dev)] if accum == 2 else [])
        reps.append((model, args, opt, sched, batches))
    (m0, a0, o0, s0, b0), (m1, a1, o1, s1, b1) = reps
    for step in range(3):
        def sync0(flat0, layout):
            def sync1(flat1, layout1):
                total = (flat0.bfloat16().float() + flat1.bfloat16().float()).bfloat16().float()
                flat0.copy_(total)
                flat1.copy_(total)
            o1.grad_sync = sync1
            with torch.enable_grad():
                for i, b in enumerate(b1):
                    U.train_step(m1, o1, s1, b, a1, step * accum + i, all_options=True)
        o0.grad_sync = sync0
        for i, b in enumerate(b0):
            U.train_step(m0, o0, s0, b, a0, step * accum + i, all_options=True)
    torch.cuda.synchronize()
    w0 = torch.cat([p.detach().reshape(-1) for p in m0.parameters()]).cpu().numpy()
    w1 = torch.cat([p.detach().reshape(-1) for p in m1.parameters()]).cpu().numpy()
    assert np.array_equal(w0, w1)
    return w0


def _run_two(mode, dtypes):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_two_rank_worker, args=(r, 2, port, q, mode, dtypes)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict((r, (s, x)) for r, s, x in (q.get(timeout=600) for _ in range(2)))
    for p in procs:
        p.join(timeout=120)
    return got, [p.exitcode for p in procs]


@pytest.mark.parametrize("mode", ["eager", "graphed", "phased", "accum"])
def test_two_gloo_ranks_equal_the_bf16_sum_emulation(dev, lib, mode):
    got, codes = _run_two(mode, ("bf16", "bf16"))
    assert all(s == "ok" for s, _ in got.values()), got
    assert codes == [0, 0]
    ref = _emulate_two_ranks(dev, mode)
    w = got[0][1]
    assert np.array_equal(w, ref), (float(np.abs(w - ref).max()), int((w != ref).sum()))


def test_mixed_exchange_dtypes_refuse_on_both_ranks_at_wrap_time(dev, lib):
    got, codes = _run_two("mixed", ("bf16", "fp32"))
    assert [got[r][0] for r in (0, 1)] == ["refused", "refused"], got
    assert all("different gradient exchange dtypes" in got[r][1] for r in (0, 1)), got
    assert codes == [0, 0]
