"""GPU, TWO OR MORE devices: the opt-in bf16 gradient exchange (DataParallel(grad_dtype="bf16")) with one rank per device over the C ABI's
RCCL communicator.  SKIPS on a one-device box, like test_rccl_multi_gpu.py; the one-device proof of the feature is
test_grad_exchange_bf16_gpu.py.

Two ranks on different batches, eager bucket hooks and the phased graphed step: every replica holds the same bits, and they equal the
single-process emulation of the bf16 sum (per-rank fp32 gradients, bf16(float(bf16(g0)) + float(bf16(g1))), AdamW with grad_scale 0.5)."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_dp_gpu import _batch, _build, _free_port
from test_grad_exchange_bf16_gpu import _emulate_two_ranks

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available() or torch.cuda.device_count() < 2,
                                 reason="needs >= 2 HIP devices: one rank per device over RCCL (the 1-GPU test box has one)")]


def _worker(rank, world, port, q, mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      HSA_ENABLE_IPC_MODE_LEGACY="0", GLOO_SOCKET_IFNAME="lo")
    os.environ.pop("YTVLN_DP_GRAD_DTYPE", None)
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "youtube-vln_amd"))
    import torch.distributed as dist
    from ytvln import distributed as D, utils_init as U
    from ytvln.vilbert_init import get_optimization
    torch.cuda.set_device(rank)
    dev = torch.device("cuda", rank)
    D.init_distributed(backend="gloo")                       # control plane only: carries the RCCL unique id
    model, args = _build(dev)
    args.learning_rate = 1e-3
    dp = D.DataParallel(model, bucket_bytes=64 << 10, collective="rccl", grad_dtype="bf16")
    assert dp.comm is not None and dp.comm.world == world and dp.bf16_exchange
    opt, sched, _, _ = get_optimization(args, model, 10, None)
    dp.attach(opt)
    batch = _batch(rank, dev)
    if mode == "eager":
        for step in range(3):
            U.train_step(dp, opt, sched, batch, args, step, all_options=True)
    else:
        U.train_step(dp, opt, sched, batch, args, 0, all_options=True)
        os.environ["YTVLN_DP_CUTS"] = "t0,c0,v1"
        gs = D.GraphedTrainStep(dp, opt, lambda backward=None: U.train_step(dp, opt, None, batch, args, 0, all_options=True, optimizer_step=False,
                                                                            backward=backward)[0],
                                bucket_bytes=64 << 10, mode="phased")
        for _ in range(2):
            loss = gs.step(sched)
        assert torch.isfinite(loss).item()
    torch.cuda.synchronize(dev)
    dp.comm.check_async_error()
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu()
    alls = [torch.zeros_like(flat) for _ in range(world)]
    dist.all_gather(alls, flat)
    same = all(torch.equal(alls[0], a) for a in alls[1:])
    dp.close()
    dist.barrier()
    dist.destroy_process_group()
    q.put((rank, same, flat.numpy() if rank == 0 else None))


@pytest.mark.parametrize("mode", ["eager", "phased"])
def test_two_devices_bf16_exchange_equals_emulation(dev, lib, mode):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, mode)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=600) for _ in range(2)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert all(same for _, same, _ in res), "replicas diverged"
    got = res[0][2]
    ref = _emulate_two_ranks(dev, mode)
    assert np.array_equal(got, ref), float(np.abs(got - ref).max())
