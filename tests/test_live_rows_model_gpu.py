"""GPU: weight gradients over the valid rows only, in the model (BertModel builds one row list per padding mask; the backward of every Linear /
FFN / image-embedding projection of that side hands it to its dW launch).  tiny_2_2_1.json, all four losses, dropout on, two-stream on,
synth.make_batch(bs=2, K=7, T=32, frames=8, boxes=12): 448 text rows and 1344 image rows, both multiples of 32, with real padding."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import CFG_DIR
from helpers import args_ns

pytestmark = pytest.mark.gpu

FLAGS = dict(ranking=True, traj_judge=True, masked_vision=True, masked_language=True)
SHAPE = dict(bs=2, K=7, T=32, frames=8, boxes=12)
GRAD_REL = 2e-4          # the project's fp32 bar: relative L2 error per tensor


def _batch(seed):
    from ytvln import synth
    nb = synth.make_batch(seed=seed, **SHAPE)
    tf, vf = float(np.asarray(nb[7]).mean()), float((np.asarray(nb[3]) > 0).mean())
    assert nb[7].size == 448 and nb[3].size == 1344
    assert tf < 0.95 and vf < 0.95, (tf, vf)          # real padding on both sides: the test cannot pass vacuously
    return nb


def _model(dev):
    from ytvln import synth
    from ytvln.lily import Lily
    from ytvln.vilbert import BertConfig
    args = args_ns(**FLAGS)
    cfg = BertConfig(**json.load(open(os.path.join(CFG_DIR, "tiny_2_2_1.json"))))
    cfg.args = args
    model = Lily(cfg, dropout_prob=0.1)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(shapes, 11).items()})
    return model.to(dev).train(), args


def _step(model, args, batch):
    """One forward + backward with the dropout stream restarted: -> (loss, {name: grad})."""
    from ytvln import ops
    from ytvln import utils_init as U
    ops.DropoutState.manual_seed(77)
    for p in model.parameters():
        p.grad = None
    loss = U.train_step(model, None, None, batch, args, 0, all_options=True, optimizer_step=False)[0]
    ops.TwoStream.join_backward()
    torch.cuda.synchronize()
    return float(loss), {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}


@pytest.fixture(scope="module")
def setup(dev, lib):
    from ytvln import ops, synth
    assert ops.get_two_stream() and ops.get_matmul_precision() == "fp32"
    model, args = _model(dev)
    return model, args, synth.to_torch(_batch(5), dev)


def test_dy_is_zero_on_listed_out_rows_at_every_site_that_gets_a_list(dev, lib, setup, monkeypatch):
    """(a) The contract of the listed launch, checked where it is used: at every backward that hands a list to its dW GEMM the A operand
    (dY, [rows, N]) is exactly zero on every row the list leaves out."""
    from ytvln import ops
    model, args, batch = setup
    seen = []

    def probe(dy, live):
        n = int(live.count.item())
        keep = torch.zeros(live.rows, dtype=torch.bool, device=dy.device)
        keep[live.idx[:n].long()] = True
        rows = dy.reshape(live.rows, -1)
        seen.append((live.rows, n, float(rows[~keep].abs().max()) if n < live.rows else 0.0, bool(torch.isfinite(rows).all())))

    monkeypatch.setattr(ops, "live_rows_probe", probe)
    _step(model, args, batch)
    sides = {r for r, _, _, _ in seen}
    assert sides == {448, 1344}, sides          # both sides' projections received lists
    # every row-wise dW launch of tiny_2_2_1: 4 self layers x (packed q|k|v, attention output, 2 of the FFN) = 16; the connection layer's
    # q1, k|v1, q2, k|v2, dense1, dense2 and two FFNs = 10; the feature projection and the fused image embedding = 2; the two heads'
    # transforms and decoders = 4
    assert len(seen) == 32, len(seen)
    assert all(n < r for r, n, _, _ in seen)
    bad = [s for s in seen if s[2] != 0.0 or not s[3]]
    assert not bad, bad[:8]


def test_one_step_with_lists_against_without(dev, lib, setup):
    """(b) GEMM_LIVE_ROWS 1 against 0: the forward is untouched (loss bit-equal); a weight gradient loses exact-zero terms and regroups its
    partial sums, so it moves by fp32 rounding."""
    from ytvln import _lib
    model, args, batch = setup
    on = _step(model, args, batch)
    prev = _lib.set_option("GEMM_LIVE_ROWS", 0)
    try:
        off = _step(model, args, batch)
    finally:
        _lib.set_option("GEMM_LIVE_ROWS", prev)
    assert on[0] == off[0], (on[0], off[0])
    # (key-projection biases have a mathematically zero gradient -- softmax shift invariance -- so both runs hold rounding noise there:
    #  the floor of tests/test_model_gpu.py, 1e-6 of the median gradient norm, takes them out of the relative comparison)
    norms = {n: float(g.double().norm()) for n, g in off[1].items() if g is not None}
    floor = 1e-6 * float(np.median(list(norms.values())))
    worst = {}
    for n, g0 in off[1].items():
        g1 = on[1][n]
        assert (g0 is None) == (g1 is None), n
        if g0 is None:
            continue
        diff = float((g1.double() - g0.double()).norm())
        assert diff <= GRAD_REL * norms[n] + floor, (n, diff, norms[n], floor)
        if norms[n] > floor:
            worst[n] = diff / norms[n]
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:3]
    print("largest relative gradient differences, lists on against off:", top, "floor", floor)
    assert any(v > 0 for v in worst.values()), "no gradient moved: the lists were not used"


def test_captured_step_follows_the_masks_of_the_batch_it_replays_on(dev, lib, setup):
    """(c) The step captured once and replayed on a second batch with other masks (copied into the static tensors) equals an eager step on
    that batch bit for bit: the list and its count are built and read on the device at replay."""
    from ytvln import ops, synth
    from ytvln import utils_init as U
    model, args, _ = setup
    first, second = _batch(5), _batch(6)
    assert not np.array_equal(first[7], second[7]) and not np.array_equal(first[3], second[3])
    static = synth.to_torch(first, dev)

    def step():
        for p in model.parameters():
            p.grad = None
        return U.train_step(model, None, None, static, args, 0, all_options=True, optimizer_step=False)[0]

    ops.DropoutState.manual_seed(77)
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss = step()
    for dst, src in zip(static, synth.to_torch(second, dev)):
        dst.copy_(src)
    state = ops.DropoutState.get_state()
    g.replay()
    torch.cuda.synchronize()
    replayed = float(loss), {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}
    ops.DropoutState.set_state(state, dev)          # the eager step draws the masks the replay drew
    eager = float(step())
    ops.TwoStream.join_backward()
    torch.cuda.synchronize()
    assert replayed[0] == eager, (replayed[0], eager)
    for n, p in model.named_parameters():
        assert (p.grad is None) == (replayed[1][n] is None) and (p.grad is None or torch.equal(p.grad, replayed[1][n])), n


def test_eval_and_no_grad_call_neither_new_entry(dev, lib, setup, monkeypatch):
    """(d) Lists are built for a training forward with gradients on, and for nothing else."""
    from ytvln import _lib, ops
    from ytvln import utils_init as U
    model, args, batch = setup
    names = []
    real = _lib.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)

    monkeypatch.setattr(_lib, "call", spy)
    monkeypatch.setattr(ops, "call", spy)          # (ops binds the function by name at import)
    new = {"ytvln_live_rows_list", "ytvln_gemm_f32_live"}
    try:
        with torch.no_grad():
            model(*U.get_model_input(batch, all_options=True))
        assert names and not (new & set(names))
        model.eval()
        model(*U.get_model_input(batch, all_options=True))
        assert not (new & set(names))
    finally:
        model.train()
    _step(model, args, batch)
    assert new <= set(names)
    assert not [n for n in names if n.startswith("ytvln_rows_")]
