"""Shared by the VILBertForVLTasks tests: the recipes of tools/gen_golden_vltasks.py restated (weights, inputs, cotangents) and an fp64
restatement of the model -- encoder and pre-training heads from oracle/vilbert_ref.py, the three new heads written out here."""
import warnings

import numpy as np
import torch
import torch.nn.functional as F

from helpers import ZERO_DROP, cfg_dict

OUT_NAMES = ("vil_prediction", "vil_logit", "vil_binary_prediction", "vision_prediction", "vision_logit", "linguisic_prediction", "linguisic_logit")
NEW_KEYS = ["vil_prediction.main.0.bias", "vil_prediction.main.0.weight_g", "vil_prediction.main.0.weight_v", "vil_prediction.main.3.bias",
            "vil_prediction.main.3.weight_g", "vil_prediction.main.3.weight_v", "vil_logit.weight", "vil_logit.bias", "vision_logit.weight",
            "vision_logit.bias", "linguisic_logit.weight", "linguisic_logit.bias"]
G_OVERRIDE = {"vil_prediction.main.0.weight_g": 1.5, "vil_prediction.main.3.weight_g": 0.75}
G_OVERRIDE_TINY = {"vil_prediction.main.0.weight_g": 13.0, "vil_prediction.main.3.weight_g": 1.5}          # about a freshly constructed model's gains
NUM_LABELS = 7
MICRO_BATCH = dict(bs=3, K=1, T=12, frames=2, boxes=5, F=16, C=11, vocab=97, seed=31)
TINY_BATCH = dict(bs=3, K=1, T=16, frames=2, boxes=4, seed=32)


def build_model(cfgname, fusion="mul", dropout_prob=0.0, **over):
    """VILBertForVLTasks on the CPU (move it with .to(dev)); with dropout_prob = 0 the two fixed dropouts of the heads (0.5 inside
    SimpleClassifier, 0.1 in front of bi_seq_relationship) are zeroed as well, as the fixtures do."""
    from ytvln.vilbert import BertConfig, VILBertForVLTasks
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", FutureWarning)
        model = VILBertForVLTasks(BertConfig(**cfg_dict(cfgname, **{**ZERO_DROP, "fusion_method": fusion, **over})), NUM_LABELS, dropout_prob=dropout_prob)
    if dropout_prob == 0.0:
        model.vil_prediction.main[2].p = model.cls.dropout.p = 0.0
    return model


def make_weights(model, seed, gains=None):
    from ytvln import synth
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    W = {k: np.asarray(v, dtype=np.float32) for k, v in synth.make_weights(shapes, seed).items()}
    for k, g in (gains or G_OVERRIDE).items():
        W[k] = np.asarray(g, dtype=np.float32)
    return W


def state_of(W, dtype=torch.float32):
    return {k: torch.as_tensor(np.asarray(v)).to(dtype).clone() for k, v in W.items()}


def inputs_of(nb, region_mask, device="cpu"):
    from ytvln import synth
    b = synth.to_torch(nb, device)
    return (b[6][:, 0], b[1][:, 0], b[2][:, 0], b[10][:, 0], b[7][:, 0].long(), torch.from_numpy(np.ascontiguousarray(region_mask)).to(device))


def cotangents(shapes, seed):
    return [(np.random.RandomState(seed + i).standard_normal(tuple(s)) / np.sqrt(max(1, int(np.prod(s))))).astype(np.float32)
            for i, s in enumerate(shapes)]


def loss_of(outs, seed, first=None):
    """L = sum_i <out_i, c_i> in fp64 (the outputs may be fp32 or bf16 device tensors); `first` replaces c_0 (the tiny fixture stores the
    cotangent of vil_prediction: noise + the gain-homogeneous part of the reference's output, see tools/gen_golden_vltasks.py)."""
    cs = cotangents([o.shape for o in outs], seed)
    if first is not None:
        cs[0] = np.asarray(first, dtype=np.float32)
    return sum((o.double() * torch.from_numpy(c).to(o.device).double()).sum() for o, c in zip(outs, cs))


def vltasks_forward(S, cfg, ids, feat, loc, type_ids, attention_mask, image_attention_mask):
    """The model with every dropout off, in the dtype of S (vilbert.py:1485-1520, 1522-1535)."""
    import vilbert_ref as O
    t, v, pt, pv = O.bert_model(S, cfg, ids, feat, loc, type_ids, attention_mask, image_attention_mask)
    lang, vis, rel = O.pretraining_heads(S, cfg, t, v, pt, pv)
    pooled = pt * pv if cfg.fusion_method == "mul" else pt + pv

    def wn(pre):
        vv = S[pre + ".weight_v"]
        return vv * (S[pre + ".weight_g"] / vv.norm())

    h = torch.relu(F.linear(pooled, wn("vil_prediction.main.0"), S["vil_prediction.main.0.bias"]))
    vil_prediction = F.linear(h, wn("vil_prediction.main.3"), S["vil_prediction.main.3.bias"])
    vil_logit = F.linear(pooled, S["vil_logit.weight"], S["vil_logit.bias"])
    vision_logit = F.linear(v, S["vision_logit.weight"], S["vision_logit.bias"]) + ((1.0 - image_attention_mask.to(v.dtype)) * -10000.0).unsqueeze(2)
    linguisic_logit = F.linear(t, S["linguisic_logit.weight"], S["linguisic_logit.bias"])
    return vil_prediction, vil_logit, rel, vis, vision_logit, lang, linguisic_logit
