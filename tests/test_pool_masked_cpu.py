"""CPU: the masked frame-pool expansions without a device.  The argument checks of ytvln.batch.expand_ragged_masked /
expand_records_masked and of the two C entry points, the host logic of the pools' expand_masked, mask_batch(vision_premasked=True) on
CPU tensors, and the invariants of the inputs the GPU tests feed (tests/pool_masked_ref.py): every decision class, both thresholds and every
bf16 tie pattern really occur, and the statement's rounding differs from truncation on them."""
import numpy as np
import pytest
import torch

from pool_masked_ref import (BF16_PATTERNS, BIG, BOXES, PADDED_DRAW, T_MASK, T_ZERO, masked_ref, ragged_case, records_case)
from ragged_pool_ref import grid_pool
from record_pool_ref import grid_records


def _ragged_inputs():
    return tuple(torch.from_numpy(a) for a in grid_pool(6, 8, 5))


def _outs(index, F=8, C=5, boxes=6, dtype=torch.float32):
    bs, K, frames = index.shape
    R = frames * boxes
    return [torch.empty(bs, K, R, F, dtype=dtype), torch.empty(bs, K, R, 12), torch.empty(bs, K, R, C), torch.empty(bs, K, R, dtype=torch.int64),
            torch.empty(bs, K, R, dtype=torch.int64)]


def test_expand_ragged_masked_checks_arguments_without_a_device():
    from ytvln.batch import expand_ragged_masked
    pf, pl, pp, offsets, index = _ragged_inputs()
    bs, K, frames = index.shape
    p = torch.zeros(bs, K, frames * 6)
    with pytest.raises(RuntimeError, match="GPU"):
        expand_ragged_masked(pf, pl, pp, offsets, index, 6)
    with pytest.raises(RuntimeError, match="GPU"):
        expand_ragged_masked(pf, pl, pp, offsets, index, 6, p=p, feature_dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU"):
        expand_ragged_masked(pf, pl, None, offsets, index, 6, masked_vision=False)
    with pytest.raises(ValueError, match="feature_dtype"):
        expand_ragged_masked(pf, pl, pp, offsets, index, 6, feature_dtype=torch.float16)
    with pytest.raises(ValueError, match="feature_dtype"):
        expand_ragged_masked(pf, pl, pp, offsets, index, 6, feature_dtype="bf16")
    with pytest.raises(ValueError, match="pool_probs"):
        expand_ragged_masked(pf, pl, None, offsets, index, 6)                       # masking without probabilities
    with pytest.raises(ValueError, match="pool_probs"):
        expand_ragged_masked(pf, pl, None, offsets, index, 6, p=p)
    with pytest.raises(ValueError, match="`p`"):
        expand_ragged_masked(pf, pl, pp, offsets, index, 6, p=p.double())
    with pytest.raises(ValueError, match="`p`"):
        expand_ragged_masked(pf, pl, pp, offsets, index, 6, p=p[:, :, :-1])
    with pytest.raises(ValueError, match="`p`"):
        expand_ragged_masked(pf, pl, pp, offsets, index, 6, p=p.reshape(bs * K, -1))
    with pytest.raises(ValueError, match="masked_vision"):
        expand_ragged_masked(pf, pl, pp, offsets, index, 6, masked_vision=False, p=p)
    with pytest.raises(ValueError, match="pool_features"):
        expand_ragged_masked(pf.double(), pl, pp, offsets, index, 6)                # the inherited checks, through the same helpers
    with pytest.raises(ValueError, match="pool_locations"):
        expand_ragged_masked(pf, torch.zeros(pf.shape[0], 12), pp, offsets, index, 6)
    with pytest.raises(ValueError, match="index"):
        expand_ragged_masked(pf, pl, pp, offsets, index.int(), 6)
    with pytest.raises(ValueError, match="boxes"):
        expand_ragged_masked(pf, pl, pp, offsets, index, 0)
    out = _outs(index)
    with pytest.raises(RuntimeError, match="GPU"):
        expand_ragged_masked(pf, pl, pp, offsets, index, 6, out=out)
    with pytest.raises(ValueError, match="image_targets_mask"):
        expand_ragged_masked(pf, pl, pp, offsets, index, 6, out=out[:4])            # the four of the unfused expansion
    with pytest.raises(ValueError, match=r"out\[0\]"):
        expand_ragged_masked(pf, pl, pp, offsets, index, 6, out=out, feature_dtype=torch.bfloat16)      # fp32 features given
    with pytest.raises(ValueError, match=r"out\[0\]"):
        expand_ragged_masked(pf, pl, pp, offsets, index, 6, out=_outs(index, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match=r"out\[0\]"):
        expand_ragged_masked(pf, pl, pp, offsets, index, 6, out=[out[0][:, :, :-1]] + out[1:])
    with pytest.raises(ValueError, match=r"out\[2\]"):
        expand_ragged_masked(pf, pl, pp, offsets, index, 6, out=out[:2] + [out[2][..., :-1].contiguous()] + out[3:])
    with pytest.raises(ValueError, match=r"out\[4\]"):
        expand_ragged_masked(pf, pl, pp, offsets, index, 6, out=out[:4] + [out[4].int()])
    with pytest.raises(ValueError, match=r"out\[3\]"):
        expand_ragged_masked(pf, pl, pp, offsets, index, 6, out=out[:3] + [out[3].int()] + out[4:])
    with pytest.raises(ValueError, match="go together"):
        expand_ragged_masked(pf, pl, pp, offsets, index, 6, out=out[:2] + [None] + out[3:])
    with pytest.raises(ValueError, match="go together"):
        expand_ragged_masked(pf, pl, pp, offsets, index, 6, out=out[:4] + [None])
    with pytest.raises(ValueError, match="go together"):
        expand_ragged_masked(pf, pl, None, offsets, index, 6, masked_vision=False, out=out)
    with pytest.raises(RuntimeError, match="GPU"):
        expand_ragged_masked(pf, pl, None, offsets, index, 6, masked_vision=False, out=[out[0], out[1], None, out[3], None])
    with pytest.raises(ValueError, match="bad"):
        expand_ragged_masked(pf, pl, pp, offsets, index, 6, bad=torch.zeros(2, dtype=torch.int64))


def test_expand_records_masked_checks_arguments_without_a_device():
    from ytvln.batch import expand_records_masked
    pf, pg, pp, offsets, index, view = (torch.from_numpy(a) for a in grid_records(6, 8, 5))
    bs, K, frames = index.shape
    glob = torch.zeros(offsets.numel() - 1, 8)
    p = torch.zeros(bs, K, frames * 6)
    with pytest.raises(RuntimeError, match="GPU"):
        expand_records_masked(pf, pg, pp, glob, offsets, index, 6, view=view, p=p, feature_dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU"):
        expand_records_masked(pf, pg, None, glob, offsets, index, 6, masked_vision=False)
    with pytest.raises(ValueError, match="feature_dtype"):
        expand_records_masked(pf, pg, pp, glob, offsets, index, 6, feature_dtype=torch.float64)
    with pytest.raises(ValueError, match="pool_probs"):
        expand_records_masked(pf, pg, None, glob, offsets, index, 6)
    with pytest.raises(ValueError, match="`p`"):
        expand_records_masked(pf, pg, pp, glob, offsets, index, 6, p=p.half())
    with pytest.raises(ValueError, match="pool_geom"):
        expand_records_masked(pf, pg[:, :6].contiguous(), pp, glob, offsets, index, 6)
    with pytest.raises(ValueError, match="pool_global"):
        expand_records_masked(pf, pg, pp, glob[:-1], offsets, index, 6)
    with pytest.raises(ValueError, match="view"):
        expand_records_masked(pf, pg, pp, glob, offsets, index, 6, view=view.float())
    out = _outs(index)
    with pytest.raises(RuntimeError, match="GPU"):
        expand_records_masked(pf, pg, pp, glob, offsets, index, 6, out=out)
    with pytest.raises(ValueError, match=r"out\[0\]"):
        expand_records_masked(pf, pg, pp, glob, offsets, index, 6, out=out, feature_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="go together"):
        expand_records_masked(pf, pg, None, glob, offsets, index, 6, masked_vision=False, out=out)
    with pytest.raises(ValueError, match="go together"):
        expand_records_masked(pf, pg, pp, glob, offsets, index, 6, out=out[:2] + [None] + out[3:4] + [None])


def test_c_entry_points_reject_bad_arguments_without_a_launch():
    from ytvln import _lib
    lib = _lib.load()
    one = 64                                                            # any non-null address: nothing is dereferenced on the host
    F32, BF16 = _lib.DT_F32, _lib.DT_BF16
    inherited = ((dict(off=None), b"null"), (dict(idx=None), b"null"), (dict(of=None), b"null"), (dict(ob=None), b"null"), (dict(om=None), b"null"),
                 (dict(pf=None), b"null"), (dict(rows=-1), b"negative"), (dict(frames_in_pool=-1), b"negative"), (dict(slots=-4), b"negative"),
                 (dict(F=-1), b"negative"), (dict(boxes=0), b"negative"), (dict(frames=0), b"frames"), (dict(slots=9), b"multiple"),
                 (dict(slots=2 ** 62), b"overflow"))
    masked = ((dict(dtype=_lib.DT_F64), b"feature_dtype"), (dict(dtype=7), b"feature_dtype"), (dict(dtype=-1), b"feature_dtype"),
              (dict(pp=None), b"masking"), (dict(ot=None, otm=None), b"masking"), (dict(pp=None, p=None, rng=one), b"masking"),
              (dict(otm=None), b"go together"), (dict(ot=None), b"go together"), (dict(p=None, ot=None), b"go together"),
              (dict(C=0), b"C > 0"), (dict(p=None, pp=None, C=0), b"C > 0"))

    ok = dict(pf=one, pl=one, pp=one, off=one, frames_in_pool=2, rows=4, idx=one, slots=8, frames=4, boxes=3, F=8, L=11, C=5, p=one, rng=None,
              site=0, of=one, dtype=F32, ob=one, ot=one, om=one, otm=one, bad=None, stream=None)

    def rc_ragged(**kw):
        a = dict(ok)
        a.update(kw)
        return lib.ytvln_expand_ragged_masked(*a.values())
    assert rc_ragged(slots=0) == 0 and rc_ragged(slots=0, dtype=BF16) == 0          # nothing to do: no launch either
    assert rc_ragged(slots=0, p=None, pp=None, ot=None, otm=None, dtype=BF16) == 0   # masking off: no probabilities, no targets
    assert rc_ragged(slots=0, p=None, pp=None) == 0                                  # masking off: targets of 1 / C need no probabilities
    for kw, word in inherited + masked + ((dict(pl=None), b"null"), (dict(L=-1), b"negative"), (dict(L=12), b"location")):
        assert rc_ragged(**kw) != 0, kw
        assert word in lib.ytvln_last_error(), (kw, lib.ytvln_last_error())

    ok = dict(pf=one, pg=one, pp=one, glob=one, off=one, frames_in_pool=2, rows=4, idx=one, view=None, slots=8, frames=4, boxes=3, F=8, C=5,
              p=one, rng=None, site=0, of=one, dtype=F32, ob=one, ot=one, om=one, otm=one, bad=None, stream=None)

    def rc_records(**kw):
        a = dict(ok)
        a.update(kw)
        return lib.ytvln_expand_records_masked(*a.values())
    assert rc_records(slots=0) == 0 and rc_records(slots=0, dtype=BF16, view=one) == 0
    assert rc_records(slots=0, p=None, pp=None, ot=None, otm=None, dtype=BF16) == 0
    for kw, word in inherited + masked + ((dict(pg=None), b"null"), (dict(glob=None), b"null")):
        assert rc_records(**kw) != 0, kw
        assert word in lib.ytvln_last_error(), (kw, lib.ytvln_last_error())


def _rows_of(p, m):
    return p[m == 1]


@pytest.mark.parametrize("case", [lambda: ragged_case("grid", 64, 21), lambda: records_case("grid", 64, 21, True),
                                  lambda: ragged_case("big", BIG["F"], BIG["C"]), lambda: records_case("big", BIG["F"], BIG["C"], False)],
                         ids=["ragged", "records", "ragged-big", "records-big"])
def test_the_draws_visit_every_class_and_both_thresholds(case):
    boxes, inp, ref, p = case()
    m = ref[3]
    real = _rows_of(p, m)
    assert (real < T_MASK).any() and ((real >= T_MASK) & (real < T_ZERO)).any() and (real >= T_ZERO).any()
    below_mask, below_zero = np.nextafter(T_MASK, np.float32(0)), np.nextafter(T_ZERO, np.float32(0))
    assert below_mask < T_MASK and T_MASK <= below_zero < T_ZERO
    for v in (T_MASK, below_mask, T_ZERO, below_zero):
        assert (real == v).any(), v
    assert T_MASK == np.float32(0.85) and T_ZERO == np.float32(0.85 + 0.15 * 0.1)      # fp32 of the reference's doubles
    pad = p[m == 0]
    assert pad.size and (pad == PADDED_DRAW).all() and PADDED_DRAW >= T_ZERO          # padded rows, padding slots: a draw that would zero and select
    bs, K, R = m.shape
    slot_p, slot_m = p.reshape(-1, boxes), m.reshape(-1, boxes)
    zero = (slot_p >= T_ZERO) & (slot_m == 1)
    sel = (slot_p >= T_MASK) & (slot_p < T_ZERO) & (slot_m == 1)
    assert (zero[:, :-1] & zero[:, 1:]).any() and (sel[:, :-1] & sel[:, 1:]).any()     # consecutive zeroed / selected rows inside one slot
    if boxes == BOXES:                                                                  # (the big shape has three real slots)
        assert zero[:, 0].any() and sel[:, 0].any()                                     # ... and as row 0 (the global region of a record slot)
    # the statement follows the classes: targets = probs exactly on the selected rows, features zero exactly on the zeroed ones
    f, bx, tg, mm, tm = masked_ref(ref, p)
    want_sel = torch.from_numpy((p >= T_MASK) & (m == 1))
    assert torch.equal(tm.bool(), want_sel) and torch.equal(tg[want_sel], torch.from_numpy(ref[2])[want_sel])
    C = ref[2].shape[-1]
    assert bool((tg[~want_sel] == torch.ones(()) / C).all())
    want_zero = torch.from_numpy((p >= T_ZERO) & (m == 1))
    assert not bool(f[want_zero].any()) and torch.equal(f[~want_zero], torch.from_numpy(ref[0])[~want_zero])
    assert bool(torch.from_numpy(ref[0])[want_zero].any())                             # rows that held something were zeroed


def test_the_big_shape_masks_a_run_across_a_piece_boundary():
    for boxes, inp, ref, p in (ragged_case("big", BIG["F"], BIG["C"]), records_case("big", BIG["F"], BIG["C"], True)):
        assert boxes == 37 and p.shape == (1, 2, 2 * 37)
        # the entry points cut 37 boxes of 4 * (2048 + 12 + 1601) (or 2 * 2048 + ...) bytes into ten pieces of four rows: rows 3 | 4 is a boundary
        for row_bytes in (4 * (2048 + 12 + 1601), 2 * 2048 + 4 * (12 + 1601)):
            want = min(37, max(4, 32768 // row_bytes))
            pieces = -(-37 // want)
            assert pieces == 10 and -(-37 // pieces) == 4
        assert p[0, 0, 3] >= T_ZERO and p[0, 0, 4] >= T_ZERO and ref[3][0, 0, 3] == 1 and ref[3][0, 0, 4] == 1
        assert ref[3][0, 1, 37:].sum() == 0                                             # a padding frame


def test_the_bf16_patterns_are_present_and_tell_rounding_from_truncation():
    bits = BF16_PATTERNS
    low, high = bits & 0xFFFF, bits >> 16
    assert (low == 0x7FFF).any() and (low == 0x8001).any() and 0x3F7FFFFF in bits.tolist()
    assert ((low == 0x8000) & (high % 2 == 0)).any() and ((low == 0x8000) & (high % 2 == 1)).any()
    assert (bits >> 31).any() and 0 in bits.tolist()
    x = torch.from_numpy(bits.view(np.float32).copy())
    rounded = x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    truncated = high.astype(np.uint16)
    half_up = ((bits.astype(np.uint64) + 0x8000) >> 16).astype(np.uint16)
    assert (rounded != truncated).any() and (rounded != half_up).any()               # nearest-even differs from both on these values
    assert rounded[bits.tolist().index(0x3F7FFFFF)] == 0x3F80                         # into the next binade
    assert rounded[bits.tolist().index(0x3F808000)] == 0x3F80 and rounded[bits.tolist().index(0x3F818000)] == 0x3F82
    for boxes, inp, ref, p in (ragged_case("grid", 5, 21), records_case("grid", 2048, 1601, False)):
        have = set(inp[0].view(np.uint32).reshape(-1).tolist())
        assert set(bits.tolist()) <= have
        shown = ref[0][ref[3] == 1].view(np.uint32)                                    # ... and they reach the output rows
        assert set(bits.tolist()) <= set(shown.reshape(-1).tolist())
        f16 = masked_ref(ref, p, bf16=True)[0]
        assert f16.dtype == torch.bfloat16
        trunc = torch.from_numpy((masked_ref(ref, p)[0].numpy().view(np.uint32) >> 16).astype(np.uint16).view(np.int16)).view(torch.bfloat16)
        assert not torch.equal(f16.view(torch.int16), trunc.view(torch.int16))


def test_mask_batch_vision_premasked_leaves_the_vision_entries_alone():
    from ytvln import batch as B
    from ytvln import synth
    b = list(synth.to_torch(synth.make_batch(bs=2, K=3, T=8, frames=2, boxes=3, F=16, C=11, vocab=97, seed=4)))
    b[1] = b[1].to(torch.bfloat16)                                      # what a pool's expand_masked(feature_dtype=torch.bfloat16) hands over
    keep = [t.clone() for t in b]
    for masked_vision in (True, False):
        out = B.mask_batch(b, masked_language=False, masked_vision=masked_vision, vision_premasked=True)
        for k in (1, 4, 5):
            assert out[k] is b[k] and torch.equal(out[k], keep[k])
        assert bool((out[8] == -1).all()) and out[6] is b[6]
        for k in range(16):
            if k != 8:
                assert torch.equal(b[k], keep[k]), k
    with pytest.raises(RuntimeError, match="GPU"):                      # the token side works as before: it has no CPU path
        B.mask_batch(b, vision_premasked=True)
    with pytest.raises(RuntimeError):                                   # and without the keyword the vision side is masked as before
        B.mask_batch([t.float() if i == 1 else t for i, t in enumerate(b)], masked_language=False)


def test_pools_expand_masked_needs_a_device_like_expand():
    from ytvln.batch import RaggedPool, RecordPool
    index = torch.zeros(1, 1, 1, dtype=torch.int64)
    ragged, record = RaggedPool(8, 2, feature_dim=8, num_classes=5), RecordPool(8, 2, feature_dim=8, num_classes=5)
    for pool in (ragged, record):
        pool.device = None                  # (a GPU may happen to be present: this test is about the host side only)
    for pool in (ragged, record):
        with pytest.raises(RuntimeError, match="GPU"):
            pool.expand(index, 4)
        with pytest.raises(RuntimeError, match="GPU"):
            pool.expand_masked(index, 4)
        with pytest.raises(RuntimeError, match="GPU"):
            pool.expand_masked(index, 4, masked_vision=False, feature_dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU"):
        record.expand_masked(index, 4, view=torch.zeros(1, 1, 1, 2, dtype=torch.float64))
