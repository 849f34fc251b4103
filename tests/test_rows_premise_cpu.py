"""CPU: the property the row-listed forward GEMMs rest on, pinned against the reference's arithmetic (oracle/vilbert_ref.py).

A listed projection returns ZEROS on the padded rows of its output instead of the values the reference computes there.  A padded row is only
ever a key behind the -10000 mask (exp gives exactly 0, and 0 * v is an exact zero for finite v), no loss reads one and the poolers read row
0: so neither the loss nor any parameter gradient may notice.  The reference's `_lin` is patched so that every output whose row count is a
side's row count has its padded rows set to zero; loss and gradients are compared with the plain run on the same batch, dropout off.

In exact terms nothing may change: what a padded row contributes to any sum is an exact zero in both runs.  The host BLAS does not quite
reproduce its own bits between the two runs, though (other buffers, other alignment: it picks other kernels): on this batch 127 of the 132
gradients are bit-equal and the five text-embedding tensors differ by at most 3.9e-7 relative, a last-place difference in a few elements.
So the loss and every gradient are held to 1e-6 relative (L2 per tensor) rather than to equality, and the counts are printed."""
import json
import os

import torch

from conftest import CFG_DIR

REL = 1e-6          # relative L2 bar per tensor where the host BLAS does not reproduce its own bits (see the docstring)


def test_zeroing_the_padded_rows_of_every_projection_changes_neither_loss_nor_gradients(monkeypatch):
    import vilbert_ref as O
    from ytvln import synth
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
    assert frac[T] < 0.95 and frac[R] < 0.95, frac          # real padding on both sides

    from ytvln.lily import Lily
    from ytvln.vilbert import BertConfig
    from helpers import args_ns
    bc = BertConfig(**cfgd)
    bc.args = args_ns(ranking=True, traj_judge=True, masked_vision=True, masked_language=True)
    shapes = {k: tuple(v.shape) for k, v in Lily(bc, dropout_prob=0.1).state_dict().items()}
    weights = synth.make_weights(shapes, 11)

    def run():
        S = O.trainable({k: torch.from_numpy(v).clone() for k, v in weights.items()})
        out = O.lily_forward(S, cfg, flags, ids, feat, loc, seg, tmask, vmask, drop=False)
        total, _ = O.total_loss(batch, out, flags)
        total.backward()
        return total.detach().clone(), {k: (None if v.grad is None else v.grad.clone()) for k, v in S.items() if isinstance(v, torch.Tensor)}

    plain = run()
    real_lin, zeroed = O._lin, []

    def _lin(S, name, x):
        y = real_lin(S, name, x)
        if y.dim() == 3 and y.shape[0] == n and y.shape[1] in valid:
            zeroed.append(y.shape[1])
            y = torch.where(valid[y.shape[1]][..., None], y, torch.zeros((), dtype=y.dtype))
        return y

    monkeypatch.setattr(O, "_lin", _lin)
    listed = run()
    assert len(zeroed) >= 40 and set(zeroed) == {T, R}, (len(zeroed), set(zeroed))
    assert abs(float(plain[0]) - float(listed[0])) <= REL * abs(float(plain[0])), (float(plain[0]), float(listed[0]))
    assert plain[1].keys() == listed[1].keys()
    seen, unequal, worst = 0, [], (0.0, None)
    for k, g0 in plain[1].items():
        g1 = listed[1][k]
        assert (g0 is None) == (g1 is None), k
        if g0 is None:
            continue
        seen += 1
        if not torch.equal(g0, g1):
            unequal.append(k)
        n0, diff = float(g0.double().norm()), float((g0.double() - g1.double()).norm())
        if n0 > 0 and diff / n0 > worst[0]:
            worst = (diff / n0, k)
        assert diff <= REL * n0, (k, diff, n0)
    print(f"{seen} gradients, {len(unequal)} not bit-equal, largest relative difference {worst}")
    assert seen > 50, seen
