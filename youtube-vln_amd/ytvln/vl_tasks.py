"""Losses and the training-step body of the downstream tasks of `VILBertForVLTasks` (answer classification, multiple choice, binary
classification, grounding), composed from the model's 7-tuple.

The wide reductions run on the library's loss kernels: the [N, num_labels] soft-target BCE and its score on `ops.bce_with_logits_rows`
(one pass over the logits gives the loss, the row arg-max and the target at it), the hard-target tasks on `ops.cross_entropy`, the
distribution over regions on `ops.kl_masked`.  Only sums and comparisons over [N]-sized tensors are torch ops, as in
`utils_init.get_loss_correct`.  Nothing here synchronises the host: losses and scores are device tensors.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import ops

Tensor = torch.Tensor
TASK_TYPES = ("VL-classifier", "VL-logit", "VL-binary-classifier", "V-logit")
# the model's outputs, in order
VIL_PREDICTION, VIL_LOGIT, VIL_BINARY_PREDICTION, VISION_PREDICTION, VISION_LOGIT, LINGUISIC_PREDICTION, LINGUISIC_LOGIT = range(7)


def _hard_target_task(logits: Tensor, target: Tensor) -> Tuple[Tensor, Tensor]:
    target = target.reshape(-1)
    loss = ops.cross_entropy(logits, target)
    score = torch.sum(torch.argmax(logits.detach(), 1) == target).float()
    return loss, score


def task_loss(task_type: str, outputs, target: Tensor, *, num_options: Optional[int] = None, v_logit_loss: str = "bce",
              pos_weight: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, int]:
    """(loss, score, batch_size) of one task from the 7-tuple `VILBertForVLTasks.forward` returns.

    "VL-classifier":        vil_prediction [N, L] against soft targets [N, L] in [0, 1]: BCE with logits summed over the labels and averaged
                            over the batch (`pos_weight`: None, one element or [L]); score = sum_r target[r, argmax_r].
    "VL-logit":             vil_logit viewed as [N / num_options, num_options] against int64 targets: cross entropy; score = #(argmax == target).
    "VL-binary-classifier": vil_binary_prediction [N, 2] against int64 targets [N]: cross entropy; score = #(argmax == target).
    "V-logit":              vision_logit viewed as [N, R] against targets [N, R] or [N, R, 1].  v_logit_loss = "bce": BCE with logits summed over
                            the regions and averaged over the batch; "kl": KLDivLoss(batchmean) of log_softmax over the regions.
                            score = #(target[r, argmax_r] > 0.5).
    `loss` is differentiable; `score` counts over the whole batch (divide by batch_size for an accuracy).  An unknown task_type, an unknown
    v_logit_loss and an N that num_options does not divide raise KeyError."""
    if task_type not in TASK_TYPES:
        raise KeyError(task_type)
    if task_type == "VL-classifier":
        x = outputs[VIL_PREDICTION]
        loss, score, _ = ops.bce_with_logits_rows(x, target, pos_weight, scale=float(x.shape[-1]))
        return loss, score, x.shape[0]
    if task_type == "VL-logit":
        x = outputs[VIL_LOGIT]
        if num_options is None or num_options <= 0 or x.numel() % num_options:
            raise KeyError(f"VL-logit: {x.numel()} logits are not rows of num_options = {num_options}")
        x = x.reshape(-1, num_options)
        return _hard_target_task(x, target) + (x.shape[0],)
    if task_type == "VL-binary-classifier":
        x = outputs[VIL_BINARY_PREDICTION]
        return _hard_target_task(x, target) + (x.shape[0],)
    if v_logit_loss not in ("bce", "kl"):
        raise KeyError(v_logit_loss)
    x = outputs[VISION_LOGIT]
    N, R = x.shape[0], x.shape[1]
    x = x.reshape(N, R)
    target = target.reshape(N, R)
    if v_logit_loss == "bce":
        loss, _, top = ops.bce_with_logits_rows(x, target, pos_weight, scale=float(R))
    else:
        loss = ops.kl_masked(x, target.float(), torch.ones(N, dtype=torch.int64, device=x.device))
        top = torch.argmax(x.detach(), 1)
    score = torch.sum(target.gather(1, top.view(-1, 1)) > 0.5).float()
    return loss, score, N


def vl_task_step(model, optimizer, scheduler, batch, task_type: str, args, step: int = 0, **task_kw) -> Tuple[Tensor, Tensor]:
    """One training iteration on one task, the counterpart of `utils_init.train_step`: forward, `task_loss`, division by
    gradient_accumulation_steps, backward, and -- every gradient_accumulation_steps -- optimizer.step(); scheduler.step(); zero_grad().
    batch = (input_txt, input_imgs, image_loc, token_type_ids, attention_mask, image_attention_mask, target).
    Returns (loss, score) as device tensors; never synchronises the host."""
    input_txt, input_imgs, image_loc, token_type_ids, attention_mask, image_attention_mask, target = batch
    outputs = model(input_txt, input_imgs, image_loc, token_type_ids, attention_mask, image_attention_mask)
    loss, score, _ = task_loss(task_type, outputs, target, **task_kw)
    accum = getattr(args, "gradient_accumulation_steps", 1)
    if accum > 1:
        loss = loss / accum
        if hasattr(model, "require_backward_grad_sync"):          # data parallel: one exchange, in the last micro-step's backward
            model.require_backward_grad_sync = (step + 1) % accum == 0
    loss.backward()
    ops.TwoStream.join_backward()
    if (step + 1) % accum == 0:
        optimizer.step()
        if scheduler is not None:
            scheduler.step()
        if hasattr(optimizer, "_arena"):
            optimizer.zero_grad()              # keeps the flat-arena views (one memset)
        else:
            model.zero_grad()
    return loss.detach(), score.detach()
