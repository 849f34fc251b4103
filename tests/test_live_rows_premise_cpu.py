"""CPU: the property the live-row weight gradients rest on, pinned against the reference's arithmetic (oracle/vilbert_ref.py).

dW = dY^T X of a Linear is contracted over the rows of the batch.  On a padded row dY is EXACTLY zero at every Linear whose rows are the text
or image rows: a padded row is a key behind the -10000 mask (exp gives exactly 0), no loss reads one, the poolers read row 0, attention
backward of a padded query row has dO = 0, and LayerNorm / GELU' / dropout backward map a zero row to a zero row.  So the products such a
row contributes are 0 * x, and with x finite they are exact zeros that need not be formed."""
import json
import os

import torch

from conftest import CFG_DIR


def test_output_gradient_of_every_row_wise_linear_is_exactly_zero_on_padded_rows(monkeypatch):
    import vilbert_ref as O
    from ytvln import synth
    torch.manual_seed(3)
    cfgd = json.load(open(os.path.join(CFG_DIR, "tiny_2_2_1.json")))
    cfg = O.RefConfig(**cfgd)
    flags = O.TaskFlags(ranking=True, traj_judge=True, masked_vision=True, masked_language=True)
    nb = synth.make_batch(bs=2, K=7, T=40, frames=8, boxes=14, seed=5)
    batch = synth.to_torch(nb)
    ids, feat, loc, seg, tmask, vmask = O.model_input(batch)
    n, T = ids.shape
    R = feat.shape[1]
    valid = {T: tmask.reshape(n, T) != 0, R: vmask.reshape(n, R) != 0}
    assert T != R
    frac = {k: float(v.float().mean()) for k, v in valid.items()}
    assert abs(frac[T] - 0.879) < 2e-3 and abs(frac[R] - 0.649) < 2e-3, frac

    from ytvln.lily import Lily
    from ytvln.vilbert import BertConfig
    from helpers import args_ns
    bc = BertConfig(**cfgd)
    bc.args = args_ns(ranking=True, traj_judge=True, masked_vision=True, masked_language=True)
    shapes = {k: tuple(v.shape) for k, v in Lily(bc, dropout_prob=0.1).state_dict().items()}
    S = O.trainable({k: torch.from_numpy(v).clone() for k, v in synth.make_weights(shapes, 11).items()})

    sites = []          # (rows per item, max |dY| over padded rows, input finite, called through _lin)
    real, real_lin, in_lin = torch.nn.functional.linear, O._lin, [False]

    def _lin(*a):
        in_lin[0] = True
        try:
            return real_lin(*a)
        finally:
            in_lin[0] = False

    def linear(x, w, b=None):
        y = real(x, w, b)
        if y.dim() == 3 and y.shape[0] == n and y.shape[1] in valid and y.requires_grad:
            rec = [y.shape[1], None, bool(torch.isfinite(x).all()), in_lin[0]]
            sites.append(rec)
            dead = ~valid[y.shape[1]]
            y.register_hook(lambda g, rec=rec, dead=dead: rec.__setitem__(1, float(g[dead].abs().max())))
        return y

    monkeypatch.setattr(torch.nn.functional, "linear", linear)
    monkeypatch.setattr(O, "_lin", _lin)
    out = O.lily_forward(S, cfg, flags, ids, feat, loc, seg, tmask, vmask, drop=True)
    total, _ = O.total_loss(batch, out, flags)
    total.backward()
    # every `_lin` of both streams, the connection layer and the heads (transforms, image decoder): 43; the tied LM decoder, which the
    # reference calls through F.linear itself, is the 44th
    assert sum(s[3] for s in sites) == 43 and len(sites) == 44, (sum(s[3] for s in sites), len(sites))
    assert {s[0] for s in sites} == {T, R}
    assert all(s[1] is not None for s in sites), "a site received no gradient"
    assert all(s[2] for s in sites), "non-finite input"
    bad = [s for s in sites if s[1] != 0.0]
    assert not bad, bad
