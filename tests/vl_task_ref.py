"""Shared by the VL-task loss tests: fp64 torch restatements of the four task losses of ytvln/vl_tasks.py and of their scores, the kernel's
BCE term written out, and the input recipe of the kernel tests."""
import numpy as np
import torch
import torch.nn.functional as F


def bce_rows_ref(x, t, pos_weight=None, scale=1.0):
    """(loss, score, row_top) in fp64: loss = scale * mean((1 - t) x + (1 + (w - 1) t) log(1 + exp(-x))), the term of the kernels;
    row_top = argmax per row (lowest index among equals), score = sum_r t[r, row_top[r]]."""
    xd, td = x.double(), t.double()
    lw = 1.0 if pos_weight is None else 1.0 + (pos_weight.double().reshape(-1) - 1.0) * td
    loss = ((1.0 - td) * xd + lw * torch.logaddexp(torch.zeros_like(xd), -xd)).mean() * scale
    top = torch.argmax(x.detach(), 1)
    return loss, td.detach().gather(1, top.view(-1, 1)).sum(), top


def _count_correct(x, target):
    return (torch.argmax(x.detach(), 1) == target.reshape(-1)).double().sum()


def task_loss_ref(task_type, outputs, target, num_options=None, v_logit_loss="bce", pos_weight=None):
    """(loss, score) of ytvln.vl_tasks.task_loss in fp64, from a 7-tuple of fp64 outputs."""
    if task_type == "VL-classifier":
        x = outputs[0]
        loss, score, _ = bce_rows_ref(x, target, pos_weight, scale=x.shape[1])
        return loss, score
    if task_type == "VL-logit":
        x = outputs[1].reshape(-1, num_options)
        return F.cross_entropy(x.double(), target.reshape(-1)), _count_correct(x, target)
    if task_type == "VL-binary-classifier":
        x = outputs[2]
        return F.cross_entropy(x.double(), target.reshape(-1)), _count_correct(x, target)
    if task_type == "V-logit":
        x = outputs[4]
        N, R = x.shape[0], x.shape[1]
        x, td = x.reshape(N, R).double(), target.reshape(N, R).double()
        if v_logit_loss == "bce":
            loss, _, top = bce_rows_ref(x, td, pos_weight, scale=R)
        else:
            loss = F.kl_div(F.log_softmax(x, 1), td, reduction="batchmean")
            top = torch.argmax(x.detach(), 1)
        return loss, (td.gather(1, top.view(-1, 1)) > 0.5).double().sum()
    raise KeyError(task_type)


SPECIAL_LOGITS = (-1e4, -50.0, 0.0, 50.0, 88.0, 1e4)
SOFT_TARGETS = (0.3, 0.6, 0.9, 1.0)


def kernel_inputs(M, C, seed, huge=True):
    """fp32 CPU (logits, targets): logits 3 N(0, 1) with 2 % of the entries replaced by values of SPECIAL_LOGITS (without the two of
    magnitude 1e4 when `huge` is False); targets 98 % zeros, the rest drawn from SOFT_TARGETS."""
    rs = np.random.RandomState(seed)
    x = (3.0 * rs.standard_normal((M, C))).astype(np.float32)
    special = np.asarray([v for v in SPECIAL_LOGITS if huge or abs(v) < 1e4], np.float32)
    pick = rs.random_sample((M, C)) < 0.02
    x[pick] = special[rs.randint(0, len(special), int(pick.sum()))]
    t = np.zeros((M, C), np.float32)
    pick = rs.random_sample((M, C)) < 0.02
    t[pick] = np.asarray(SOFT_TARGETS, np.float32)[rs.randint(0, len(SOFT_TARGETS), int(pick.sum()))]
    return torch.from_numpy(x), torch.from_numpy(t)
