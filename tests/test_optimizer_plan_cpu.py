"""CPU: which C entry points a step of the arena AdamW issues, in which order, for every combination of its opt-in features (gradient
clipping, LAMB trust ratio, weight EMA, per-tensor statistics) and both gradient operands -- the eager form (`_launch_kernels`) and the
grouped form of the phased data-parallel step (`group_update` per gradient group, then `finish_group_step`).  `ops.call` is recorded, not
run: the stub of tests/test_ema_cpu.py, two launch classes of one chunk record each."""
import itertools

import pytest
import torch

from test_ema_cpu import _stubbed

LAMB = ["ytvln_lamb_stage1", "ytvln_lamb_trust", "ytvln_lamb_stage2"]
STATS = ["ytvln_tensor_stats_stage1", "ytvln_tensor_stats_stage2"]
ON = {"clip": {"max_grad_norm": 1.0}, "lamb": {"trust_ratio": True}, "ema": {"ema_decay": 0.9}, "stats": {"tensor_stats": True}}
COMBOS = list(itertools.product([False, True], repeat=4))          # (clip, lamb, ema, stats)


def _plan_opt(monkeypatch, clip=False, lamb=False, ema=False, stats=False, bf16=False):
    from ytvln import ops
    attrs = {}
    for name, on in (("clip", clip), ("lamb", lamb), ("ema", ema), ("stats", stats)):
        if on:
            attrs.update(ON[name])
    opt, seen = _stubbed(monkeypatch, **attrs)
    monkeypatch.setattr(ops, "_check_stats_partials", lambda *a, **k: None)
    opt._arena.setdefault("stats", None)
    if bf16:                                   # the update reads the bf16 sums of the bf16 exchange
        opt.exchange_dtype = torch.bfloat16
        opt._arena["gb"] = torch.zeros(16, dtype=torch.bfloat16)
    return opt, seen


def _update(clip, lamb, ema, bf16=False, copy=False):
    """The launches that update one chunk table."""
    if lamb:
        names = list(LAMB)
    elif clip:
        names = ["ytvln_adamw_clip"]
    elif bf16:
        names = ["ytvln_adamw_f32_gbf16"]
    else:
        names = ["ytvln_adamw_f32_bf16copy" if copy else "ytvln_adamw_f32"]
    return names + (["ytvln_ema_update"] if ema else [])


def _eager(opt, seen):
    opt._upload_hyper()
    opt._launch_kernels()
    return [n for n, _ in seen]


# ---- 1. the eager plan ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["g_f32", "g_bf16"])
@pytest.mark.parametrize("clip,lamb,ema,stats", COMBOS)
def test_eager_plan(monkeypatch, clip, lamb, ema, stats, bf16):
    opt, seen = _plan_opt(monkeypatch, clip, lamb, ema, stats, bf16)
    classes = len(opt._launch)
    want = (["ytvln_grad_sumsq"] * classes + ["ytvln_grad_clip_coef"] if clip else []) + _update(clip, lamb, ema, bf16) * classes + \
        (STATS * classes if stats else [])
    assert _eager(opt, seen) == want


def test_eager_plan_of_the_plain_update_with_a_bf16_weight_copy(monkeypatch):
    opt, seen = _plan_opt(monkeypatch)
    opt._arena["pb"] = torch.zeros(16, dtype=torch.bfloat16)
    assert _eager(opt, seen) == ["ytvln_adamw_f32_bf16copy"] * 2


# ---- 2. the grouped plan ----------------------------------------------------------------------------------------------------------------------
def _groups(opt):
    """Two gradient groups that cut the two launch classes apart: the form of group_tables(), one table each (copies, as there)."""
    return [[(ci, c["table"].clone(), c["n"])] for ci, c in enumerate(opt._launch)]


@pytest.mark.parametrize("clip,lamb,ema,stats", COMBOS)
def test_grouped_plan(monkeypatch, clip, lamb, ema, stats):
    opt, seen = _plan_opt(monkeypatch, clip, lamb, ema, stats)
    tables = _groups(opt)
    ntables, classes, records = sum(len(t) for t in tables), len(opt._launch), sum(n for t in tables for _, _, n in t)
    update, report = _update(clip, lamb, ema), (STATS * classes if stats else [])
    if clip:          # per group only the sums of squares; the coefficient and every update wait for the last group's partials
        want_groups = [["ytvln_grad_sumsq"] * len(t) for t in tables]
        want_finish = ["ytvln_grad_clip_coef"] + update * (classes if lamb else ntables) + report
    elif lamb:        # the norms run over whole tensors: every update waits for the last group
        want_groups, want_finish = [[] for _ in tables], update * classes + report
    else:
        want_groups, want_finish = [update * len(t) for t in tables], report
    group_ptrs = [table.data_ptr() for t in tables for _, table, _ in t]
    chunks_of = {"ytvln_grad_sumsq": 2, "ytvln_adamw_clip": 6, "ytvln_adamw_f32": 4, "ytvln_lamb_stage1": 5}    # the chunk table's argument
    for replay in range(2):                    # a second prepare_replay() starts the partial slots at 0 again
        del seen[:]
        opt._written.add(1)
        opt.prepare_replay()
        assert seen == []
        cuts = [0]
        for t in tables:
            opt.group_update(t)
            cuts.append(len(seen))
        opt.finish_group_step(tables)
        names = [n for n, _ in seen]
        assert [names[lo:hi] for lo, hi in zip(cuts, cuts[1:])] == want_groups
        assert names[cuts[-1]:] == want_finish
        chunks = {name: [a[chunks_of[name]] for n, a in seen if n == name] for name in chunks_of}
        if clip:      # each table in its turn into the next free slots; the coefficient over all the slots that were filled
            base = opt._arena["partials"].data_ptr()
            assert chunks["ytvln_grad_sumsq"] == group_ptrs
            assert [a[4] for n, a in seen if n == "ytvln_grad_sumsq"] == [base + 4 * i for i in range(records)]
            assert [a[:2] for n, a in seen if n == "ytvln_grad_clip_coef"] == [(base, records)]
        if lamb:      # over the launch classes' own tables, not the groups' cuts of them
            assert chunks["ytvln_lamb_stage1"] == [c["table"].data_ptr() for c in opt._launch]
        else:         # every group's table, in group order
            assert chunks["ytvln_adamw_clip" if clip else "ytvln_adamw_f32"] == group_ptrs
        assert opt._written == set()


# ---- 3. capture_buffers ------------------------------------------------------------------------------------------------------------------------
KEYS = {"clip": ("partials", "clip"), "lamb": ("lamb",), "ema": ("ema",), "stats": ("stats",), "bf16": ("gb",)}


@pytest.mark.parametrize("feature", [None] + sorted(KEYS))
def test_capture_buffers_allocates_what_the_settings_need_and_nothing_else(monkeypatch, feature):
    opt, seen = _plan_opt(monkeypatch, **({feature: True} if feature and feature != "bf16" else {}))
    if feature == "bf16":
        opt.exchange_dtype = torch.bfloat16
    opt.capture_buffers()
    a = opt._arena
    want = set(KEYS[feature]) if feature else set()
    assert {k for keys in KEYS.values() for k in keys if a[k] is not None} == want
    assert seen == []                          # allocation only: nothing is launched
