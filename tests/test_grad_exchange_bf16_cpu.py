"""CPU: choosing the element type of the data-parallel gradient exchange (DataParallel(grad_dtype=...) / YTVLN_DP_GRAD_DTYPE).

fp32 stays the default everywhere; bf16 is opt-in, and since its pack and update are HIP kernels a module that is not on a HIP device is
refused instead of running some other path."""
import pytest
import torch
from torch import nn


@pytest.fixture
def D(monkeypatch):
    monkeypatch.delenv("YTVLN_DP_GRAD_DTYPE", raising=False)
    from ytvln import distributed
    return distributed


def test_default_is_fp32(D):
    assert D.grad_exchange_dtype() is torch.float32
    assert D.grad_exchange_dtype(None) is torch.float32


@pytest.mark.parametrize("value,want", [("fp32", torch.float32), ("bf16", torch.bfloat16),
                                        (torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16)])
def test_argument_forms(D, value, want):
    assert D.grad_exchange_dtype(value) is want


@pytest.mark.parametrize("value,want", [("fp32", torch.float32), ("bf16", torch.bfloat16)])
def test_environment_variable(D, monkeypatch, value, want):
    monkeypatch.setenv("YTVLN_DP_GRAD_DTYPE", value)
    assert D.grad_exchange_dtype() is want
    assert D.grad_exchange_dtype("fp32") is torch.float32          # an explicit argument wins over the variable


@pytest.mark.parametrize("value", ["fp16", "BF16", "float32", "", torch.float16, torch.float64])
def test_bad_values_raise(D, monkeypatch, value):
    with pytest.raises(ValueError, match="expected 'fp32' or 'bf16'"):
        D.grad_exchange_dtype(value)
    if isinstance(value, str):
        monkeypatch.setenv("YTVLN_DP_GRAD_DTYPE", value)
        with pytest.raises(ValueError):
            D.grad_exchange_dtype()
        with pytest.raises(ValueError):
            D.DataParallel(nn.Linear(4, 4))


def test_bf16_refused_on_a_cpu_module(D, monkeypatch):
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        D.DataParallel(nn.Linear(4, 4), grad_dtype="bf16")
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        D.DataParallel(nn.Linear(4, 4), grad_dtype=torch.bfloat16)
    monkeypatch.setenv("YTVLN_DP_GRAD_DTYPE", "bf16")
    with pytest.raises(RuntimeError, match="not on a HIP device"):
        D.DataParallel(nn.Linear(4, 4))


def test_fp32_cpu_module_unchanged(D, monkeypatch):
    monkeypatch.setenv("YTVLN_DP_GRAD_DTYPE", "fp32")
    dp = D.DataParallel(nn.Linear(4, 4))
    assert dp.grad_dtype is torch.float32 and not dp.bf16_exchange
    assert dp.exchange_bytes_per_step() == 0                        # one rank, no always_exchange: nothing travels
    opt = torch.optim.SGD(dp.parameters(), lr=0.1)
    dp.attach(opt)
    assert opt.exchange_dtype is torch.float32 and opt.grad_scale == 1.0
    dp.close()


def test_adamw_allocates_no_exchange_buffer_by_default():
    from ytvln.optimization import AdamW
    opt = AdamW([nn.Parameter(torch.zeros(4))], lr=1e-3)
    assert opt.exchange_dtype is torch.float32 and opt.grad_bf16() is None
    assert "gb" not in opt.state_dict()["state"]
