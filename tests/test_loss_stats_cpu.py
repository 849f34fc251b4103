"""CPU: label smoothing and same-pass accuracy of the CE / KL loss kernels -- everything that needs no device: the fp64 restatement
(tests/loss_stats_ref.py) against torch, the argument checks of ops and of the two args fields, and the entry points' own refusals."""
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_stats_ref as R

ENTRY_POINTS = ["ytvln_ce_stats_fwd_f32", "ytvln_ce_stats_fwd_bf16", "ytvln_ce_smooth_bwd_f32", "ytvln_ce_smooth_bwd_bf16",
                "ytvln_kl_stats_fwd_f32", "ytvln_kl_stats_fwd_bf16"]


def _case(M, V, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, V, generator=g, dtype=torch.float64) * 2.0
    t = torch.randint(0, V, (M,), generator=g)
    t[::3] = -1
    return x, t


@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("M,V", [(1, 2), (5, 7), (30, 257)])
def test_ce_restatement_is_torch_cross_entropy_where_no_logit_is_minus_inf(M, V, eps):
    x, t = _case(M, V, seed=M + V)
    if M == 1:
        t[0] = 1
    xr = x.clone().requires_grad_(True)
    want = F.cross_entropy(xr, t, ignore_index=-1, label_smoothing=eps)
    (want * 3.0).backward()
    got = R.ce_stats(x.numpy(), t.numpy(), -1, eps, gout=3.0)
    want = float(want.detach())
    assert abs(got["loss"] - want) <= 1e-12 * max(1.0, abs(want))
    assert np.abs(got["grad"] - xr.grad.numpy()).max() <= 1e-12
    live = (t != -1).numpy()
    assert got["count"] == int(live.sum())
    top = x.argmax(-1).numpy()
    assert np.array_equal(got["row_top"], np.where(live, top, -1))
    assert got["hits"] == int((live & (top == t.numpy())).sum())


@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5])
def test_ce_restatement_with_minus_inf_padding_is_torch_on_the_finite_sub_row(eps):
    """ranking-style rows [bs, 7]: the options beyond a row's own number are -inf; torch on the whole row gives +inf with smoothing on"""
    x, _ = _case(6, 7, seed=11)
    widths = [7, 3, 5, 2, 4, 6]
    t = torch.tensor([0, 2, -1, 1, 3, 5])
    for r, w in enumerate(widths):
        x[r, w:] = -math.inf
    got = R.ce_stats(x.numpy(), t.numpy(), -1, eps)
    live = [r for r in range(6) if t[r] != -1]
    want_rows, want_grad = [], np.zeros((6, 7))
    for r in live:
        sub = x[r:r + 1, :widths[r]].clone().requires_grad_(True)
        l = F.cross_entropy(sub, t[r:r + 1], label_smoothing=eps)
        l.backward()
        want_rows.append(float(l))
        want_grad[r, :widths[r]] = sub.grad.numpy()[0] / len(live)
    assert np.abs(got["row_loss"][live] - np.array(want_rows)).max() <= 1e-12
    assert abs(got["loss"] - sum(want_rows) / len(live)) <= 1e-12
    assert np.abs(got["grad"] - want_grad).max() <= 1e-12
    assert np.all(got["grad"][np.isneginf(x.numpy())] == 0.0)
    if eps > 0:
        assert math.isinf(float(F.cross_entropy(x, t, ignore_index=-1, label_smoothing=eps)))       # the documented difference


def test_ce_restatement_special_rows():
    x, t = _case(4, 9, seed=5)
    t[:] = torch.tensor([1, 2, 3, 4])
    x[0, 5] = x[0, 2] = x[0].max() + 1.0            # equal maxima: the lowest index
    x[1, 6] = x[1, 3] = math.nan                    # NaN counts as the maximum: the first NaN; the loss of that row alone is NaN
    x[2, 3] = -math.inf                             # the target's own logit is -inf: +inf
    got = R.ce_stats(x.numpy(), t.numpy(), -1, 0.1)
    assert list(got["row_top"][:2]) == [2, 3]
    assert math.isnan(got["row_loss"][1]) and got["row_loss"][2] == math.inf and math.isfinite(got["row_loss"][0]) and math.isfinite(got["row_loss"][3])
    assert np.isfinite(got["grad"][[0, 3]]).all() and np.isnan(got["grad"][1]).all()
    none = R.ce_stats(x.numpy(), np.full(4, -1), -1, 0.1)
    assert math.isnan(none["loss"]) and none["hits"] == 0 and none["count"] == 0 and list(none["row_top"]) == [-1] * 4
    bad = R.ce_stats(x.numpy(), np.array([1, 9, 3, 4]), -1, 0.0)
    assert math.isnan(bad["row_loss"][1])


@pytest.mark.parametrize("frac", [0.0, 0.4, 1.0])
def test_kl_restatement_is_the_masked_kl_div_expression(frac):
    g = torch.Generator().manual_seed(3)
    M, C = 12, 37
    x = torch.randn(M, C, generator=g, dtype=torch.float64)
    tt = torch.softmax(torch.randn(M, C, generator=g, dtype=torch.float64) * 3, -1)
    tt[2, 5:9] = 0.0                                # xlogy: a zero target adds nothing
    mk = (torch.rand(M, generator=g) < frac).long()
    xr = x.clone().requires_grad_(True)
    want = (F.kl_div(F.log_softmax(xr, -1), tt, reduction="none") * mk.unsqueeze(-1).double()).sum() / max(1, int(mk.sum()))
    want.backward()
    got = R.kl_stats(x.numpy(), tt.numpy(), mk.numpy())
    assert abs(got["loss"] - float(want.detach())) <= 1e-12
    assert np.abs(got["grad"] - xr.grad.numpy()).max() <= 1e-12
    on = mk.numpy() != 0
    assert got["count"] == int(on.sum())
    assert got["hits"] == int((on & (x.argmax(-1) == tt.argmax(-1)).numpy()).sum())
    assert np.array_equal(got["row_top"], np.where(on, x.argmax(-1).numpy(), -1))


BAD_SMOOTHING = [-0.1, 1.0, 1.5, float("nan"), float("inf"), "0.1", None, True, 1j]


@pytest.mark.parametrize("bad", BAD_SMOOTHING, ids=repr)
def test_ops_refuse_an_invalid_label_smoothing_before_any_launch(bad, monkeypatch):
    from ytvln import _lib, ops
    monkeypatch.setattr(ops, "call", lambda *a, **k: pytest.fail("a kernel was launched"))
    x, t = torch.zeros(4, 8), torch.zeros(4, dtype=torch.long)          # CPU tensors: the value is checked first
    with pytest.raises(ValueError, match="label_smoothing"):
        ops.cross_entropy(x, t, -1, label_smoothing=bad)
    with pytest.raises(ValueError, match="label_smoothing"):
        ops.cross_entropy_stats(x, t, -1, bad)
    assert _lib is not None


def test_ops_refuse_cpu_tensors_and_keep_their_signatures():
    import inspect
    from ytvln import ops
    x, t = torch.zeros(4, 8), torch.zeros(4, dtype=torch.long)
    for fn in (lambda: ops.cross_entropy(x, t, -1, label_smoothing=0.1), lambda: ops.cross_entropy_stats(x, t, -1),
               lambda: ops.cross_entropy_stats(x, t, -1, 0.1), lambda: ops.kl_masked_stats(x, x, t)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()
    assert list(inspect.signature(ops.cross_entropy).parameters) == ["logits", "target", "ignore_index", "label_smoothing"]
    assert inspect.signature(ops.cross_entropy).parameters["label_smoothing"].default == 0.0
    assert list(inspect.signature(ops.cross_entropy_stats).parameters) == ["logits", "target", "ignore_index", "label_smoothing"]
    assert list(inspect.signature(ops.kl_masked_stats).parameters) == ["pred", "target", "mask"]


def _args(**over):
    a = types.SimpleNamespace(model_name="vilbert", ranking=True, traj_judge=True, masked_vision=True, masked_language=True, pretrain=True,
                              num_negatives=2, traj_loss_scale=1.0, not_traj_judge_data=False, gradient_accumulation_steps=1, local_rank=-1,
                              skip_all_reduce=True)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_the_two_args_fields_default_off_and_are_validated_when_the_step_runs():
    from ytvln import utils_init as U
    assert U.loss_settings(_args()) == (0.0, False)
    assert U.loss_settings(_args(label_smoothing=0.1, token_accuracy=True)) == (0.1, True)
    assert U.loss_settings(_args(label_smoothing=0)) == (0.0, False)
    for bad in BAD_SMOOTHING:
        with pytest.raises(ValueError, match="label_smoothing"):
            U.loss_settings(_args(label_smoothing=bad))
        with pytest.raises(ValueError, match="label_smoothing"):          # the step itself: refused before the model is touched
            U.train_step(None, None, None, None, _args(label_smoothing=bad))
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="token_accuracy"):
            U.loss_settings(_args(token_accuracy=bad))
        with pytest.raises(ValueError, match="token_accuracy"):
            U.train_step(None, None, None, None, _args(token_accuracy=bad))


def _fwd_args(name, **over):
    """a well-formed argument list of a stats entry point with made-up (never dereferenced) addresses; `over` breaks one of them"""
    p = 4096
    if "kl_stats" in name:
        a = dict(pred=p, ld=16, target=p, ldt=16, mask=p, row_lse=p, row_loss=p, row_top=p, row_hit=p, out=p, M=4, C=16, stream=None)
    elif "stats_fwd" in name:
        a = dict(logits=p, ld=16, target=p, ignore=-1, eps=0.1, row_lse=p, row_aux=p, row_loss=p, row_top=p, out=p, M=4, V=16, stream=None)
    else:
        a = dict(logits=p, ld=16, target=p, ignore=-1, eps=0.1, row_lse=p, row_aux=p, out=p, gout=p, dlogits=p, ldd=16, M=4, V=16, stream=None)
    a.update(over)
    return list(a.values())


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_entry_points_reject_bad_arguments_without_a_device(name):
    """every call below is refused by the host-side checks: nothing is launched, no pointer is read"""
    from ytvln import _lib
    lib = _lib.load()
    fn = getattr(lib, name)
    cases = [dict(M=0), dict(M=-3), dict(M=(1 << 24) + 1), dict(ld=15), dict(target=None), dict(out=None), dict(row_lse=None)]
    cases.append(dict(pred=None) if "kl_stats" in name else dict(logits=None))
    if "kl_stats" in name:
        cases += [dict(ldt=15), dict(row_top=None), dict(row_hit=None), dict(mask=None)]
    else:
        cases += [dict(eps=-0.1), dict(eps=1.0), dict(eps=float("nan")), dict(eps=float("inf")), dict(row_aux=None)]
        cases += [dict(ldd=15), dict(gout=None), dict(dlogits=None)] if "bwd" in name else [dict(row_top=None), dict(row_loss=None)]
    for over in cases:
        rc = fn(*_fwd_args(name, **over))
        assert rc < 0, (name, over)
        msg = lib.ytvln_last_error().decode()
        assert name[len("ytvln_"):] in msg, (name, over, msg)
    with pytest.raises(RuntimeError, match=name + " failed"):
        _lib.call(name, *_fwd_args(name, M=0))
