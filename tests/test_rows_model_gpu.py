"""GPU: forward and input-gradient GEMMs on the valid rows only, in the model (run-time option GEMM_LIVE_M; BertModel hands the row
permutation of each padding mask to the transA = 0 launches of that side's LinearFn / FFNFn).  The tiny model, batch and step of
tests/test_live_rows_model_gpu.py: tiny_2_2_1.json, all four losses, dropout on, two-stream on, 448 text rows and 1344 image rows with real
padding.  The hints are pinned (BertModel.rows_hint) so that every run of a comparison plans its launches alike: 256 text rows and 768 image
rows, both below the row counts (at the row count a side passes no list at all).  The forward GEMMs are listed only where the model says so
(BertModel.forward_live_rows, off by default because the zeros reach the padded rows of the model's outputs): tests (a)-(c) switch it on, (d)
checks the default, in which only the input-gradient launches take the list and nothing at all changes."""
import numpy as np
import pytest
import torch

from test_live_rows_model_gpu import GRAD_REL, _batch, _model, _step

pytestmark = pytest.mark.gpu

HINT = (256, 768)


@pytest.fixture(scope="module")
def setup(dev, lib):
    from ytvln import ops, synth
    assert ops.get_two_stream() and ops.get_matmul_precision() == "fp32"
    model, args = _model(dev)
    model.bert.rows_hint = HINT
    model.bert.forward_live_rows = True
    return model, args, synth.to_torch(_batch(5), dev)


def _valid(batch, dev):
    """(text, image) bool masks [N, rows per item] of the pairs the model sees."""
    from ytvln import utils_init as U
    inp = U.get_model_input(batch, all_options=True)
    return inp[4] != 0, inp[5] != 0


def test_one_step_with_the_option_on_against_off(dev, lib, setup):
    """(a) GEMM_LIVE_M 1 against 0.  Both runs take the same splits by construction -- a listed launch keeps the split count of the unlisted
    one (asserted below through the two plan entry points on the shapes that can split) -- so a valid row carries the same bits.  The padded
    rows of every projection become zeros, which only ever were keys behind the mask: the loss agrees to 1e-6, every gradient within the
    project's fp32 bar, and the sequence outputs are finite everywhere and bit-equal on the valid rows."""
    import ctypes
    for M, hint in ((448, HINT[0]), (1344, HINT[1])):
        for N, K in ((256, 256), (512, 256), (256, 512), (256, 2048)):
            tm, tn, sp, sp0 = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            assert lib.ytvln_gemm_rows_plan(M, N, K, 0, hint, ctypes.byref(tm), ctypes.byref(tn), ctypes.byref(sp)) == 0
            assert lib.ytvln_gemm_plan(M, N, K, 0, 0, ctypes.byref(tm), ctypes.byref(tn), ctypes.byref(sp0)) == 0
            assert sp.value == sp0.value, (M, N, K, sp.value, sp0.value)
    from ytvln import _lib
    model, args, batch = setup
    seqs = []
    hook = model.bert.register_forward_hook(lambda mod, a, out: seqs.append((out[0].detach().clone(), out[1].detach().clone())))
    try:
        on = _step(model, args, batch)
        prev = _lib.set_option("GEMM_LIVE_M", 0)
        try:
            off = _step(model, args, batch)
        finally:
            _lib.set_option("GEMM_LIVE_M", prev)
    finally:
        hook.remove()
    assert len(seqs) == 2
    vt, vv = _valid(batch, dev)
    for side, valid in ((0, vt), (1, vv)):
        a, b = seqs[0][side], seqs[1][side]
        assert a.shape[:2] == valid.shape, (a.shape, valid.shape)
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
        assert torch.equal(a[valid], b[valid]), ("sequence output differs on valid rows", side, float((a[valid] - b[valid]).abs().max()))
        assert not torch.equal(a[~valid], b[~valid]), "padded rows did not change: the lists were not used"
    print("loss, option on / off:", on[0], off[0])
    assert abs(on[0] - off[0]) <= 1e-6 * abs(off[0]), (on[0], off[0])
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
    print("largest relative gradient differences, option on against off:", sorted(worst.items(), key=lambda kv: -kv[1])[:3], "floor", floor)


def test_captured_step_follows_the_masks_of_the_batch_it_replays_on(dev, lib, setup):
    """(b) The step captured on one batch and replayed on a second batch with other masks equals an eager step on that batch bit for bit: the
    permutation and its count are built and read on the device at replay, and the grid never depended on the count."""
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
    ops.DropoutState.set_state(state, dev)
    eager = float(step())
    ops.TwoStream.join_backward()
    torch.cuda.synchronize()
    assert replayed[0] == eager, (replayed[0], eager)
    for n, p in model.named_parameters():
        assert (p.grad is None) == (replayed[1][n] is None) and (p.grad is None or torch.equal(p.grad, replayed[1][n])), n


def test_eval_and_no_grad_call_none_of_the_new_entries(dev, lib, setup, monkeypatch):
    """(c) Lists are built for a training forward with gradients on, and for nothing else; a training step hands them to launches of both
    sides' row counts, forward (B = [N, K]) and input gradient (B = [K, N])."""
    from ytvln import _lib, ops
    from ytvln import utils_init as U
    model, args, batch = setup
    calls = []
    real = _lib.call

    def spy(name, *a):
        calls.append((name, a))
        return real(name, *a)

    monkeypatch.setattr(_lib, "call", spy)
    monkeypatch.setattr(ops, "call", spy)          # (ops binds the function by name at import)
    new = {"ytvln_live_rows_perm", "ytvln_gemm_f32_rows"}
    try:
        with torch.no_grad():
            model(*U.get_model_input(batch, all_options=True))
        assert calls and not (new & {n for n, _ in calls})
        model.eval()
        model(*U.get_model_input(batch, all_options=True))
        assert not (new & {n for n, _ in calls})
    finally:
        model.train()
    _step(model, args, batch)
    assert new <= {n for n, _ in calls}
    # ytvln_gemm_f32_rows(A, lda, transA, B, ldb, transB, C, ldc, bias, aux, ldaux, M, ...): (M, transB) of every listed launch
    seen = {(a[11], a[5]) for n, a in calls if n == "ytvln_gemm_f32_rows"}
    assert seen == {(448, 1), (448, 0), (1344, 1), (1344, 0)}, seen
    assert all(a[2] == 0 for n, a in calls if n == "ytvln_gemm_f32_rows")
    assert {a[21] for n, a in calls if n == "ytvln_gemm_f32_rows"} == set(HINT)


def test_default_lists_only_the_input_gradients_and_changes_nothing(dev, lib, setup, monkeypatch):
    """(d) forward_live_rows off (the default): only launches with B = [K, N] (input gradients) take the list, and against GEMM_LIVE_M = 0 the
    loss, the sequence outputs on EVERY row and every gradient are equal -- dY is zero on a padded row, so the rows left out were zeros."""
    from ytvln import _lib, ops
    model, args, batch = setup
    seqs, calls = [], []
    real = _lib.call

    def spy(name, *a):
        calls.append((name, a))
        return real(name, *a)

    hook = model.bert.register_forward_hook(lambda mod, a, out: seqs.append((out[0].detach().clone(), out[1].detach().clone())))
    model.bert.forward_live_rows = False
    try:
        monkeypatch.setattr(_lib, "call", spy)
        monkeypatch.setattr(ops, "call", spy)
        on = _step(model, args, batch)
        monkeypatch.undo()
        prev = _lib.set_option("GEMM_LIVE_M", 0)
        try:
            off = _step(model, args, batch)
        finally:
            _lib.set_option("GEMM_LIVE_M", prev)
    finally:
        model.bert.forward_live_rows = True
        hook.remove()
    seen = {(a[11], a[5]) for n, a in calls if n == "ytvln_gemm_f32_rows"}
    assert seen == {(448, 0), (1344, 0)}, seen
    assert on[0] == off[0], (on[0], off[0])
    for side in (0, 1):
        assert torch.equal(seqs[0][side], seqs[1][side]), side
    for n, g0 in off[1].items():
        g1 = on[1][n]
        assert (g0 is None) == (g1 is None) and (g0 is None or torch.equal(g0, g1)), n


def test_recompute_tiers_with_the_forward_listed(dev, lib, setup):
    """(e) forward_live_rows with BertEncoder.recompute = "ffn" / "layer": the recomputed forward runs unlisted (its padded rows hold other
    values, still only keys behind the mask), so loss and gradients are those of recompute = "none" within the project's fp32 bar."""
    model, args, batch = setup
    enc = model.bert.encoder
    base = _step(model, args, batch)
    norms = {n: float(g.double().norm()) for n, g in base[1].items() if g is not None}
    floor = 1e-6 * float(np.median(list(norms.values())))
    try:
        for tier in ("ffn", "layer"):
            enc.recompute = tier
            got = _step(model, args, batch)
            assert abs(got[0] - base[0]) <= 1e-6 * abs(base[0]), (tier, got[0], base[0])
            for n, g0 in base[1].items():
                g1 = got[1][n]
                assert (g0 is None) == (g1 is None), (tier, n)
                if g0 is not None:
                    diff = float((g1.double() - g0.double()).norm())
                    assert diff <= GRAD_REL * norms[n] + floor, (tier, n, diff, norms[n])
    finally:
        enc.recompute = "none"


def test_the_posted_count_becomes_the_next_forwards_hint_and_capture_posts_nothing(dev, lib, setup):
    """(f) BertModel.rows_hint = None: the first forward plans without a count and posts it; a later forward that finds the copy complete
    uses it rounded up to 256 rows (capped at the rows of the side).  Under capture the last value is returned and nothing is posted or queried."""
    from ytvln import utils_init as U
    from ytvln.vilbert import _RowsHint
    model, args, batch = setup
    vt, vv = _valid(batch, dev)
    want = tuple(-(-int(v.sum()) // 256) * 256 for v in (vt, vv))
    model.bert.rows_hint, model.bert._rows_hints = None, None
    try:
        _step(model, args, batch)          # (ends with a synchronize: the posted copies are complete)
        assert all(h.value == 0 and h.event is not None for h in model.bert._rows_hints)
        _step(model, args, batch)
        assert tuple(h.value for h in model.bert._rows_hints) == want, ([h.value for h in model.bert._rows_hints], want)
        assert tuple(lr.hint for lr in model.bert.live_rows) == (min(want[0], 448), min(want[1], 1344))
    finally:
        model.bert.rows_hint = HINT
    h = _RowsHint()
    h.value = 512
    count = torch.tensor([300], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = h.step(count)
        count.add_(0)          # (a graph needs a node)
    assert got == 512 and h.event is None and h.pinned is None
