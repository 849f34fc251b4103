"""CPU: the host side of the stored-dS attention backward (include/ytvln.h: ytvln_attn_bwd_workspace_elems, ytvln_attn_bwd_ws_f32,
ytvln_attn_bwd_pair_ws).  The size query is pure host code and decides exactly as the launch does: 0 means "the recomputing kernels"."""
import math
import subprocess

import pytest

from test_abi import ctype_of, header_decls

NEW = ("ytvln_attn_bwd_workspace_elems", "ytvln_attn_bwd_ws_f32", "ytvln_attn_bwd_pair_ws")


@pytest.fixture
def options():
    from ytvln import _lib
    prev = {}

    def set_(**kw):
        for k, v in kw.items():
            p = _lib.set_option(k, v)
            prev.setdefault(k, p)
    yield set_
    for k, v in prev.items():
        _lib.set_option(k, v)


def blocks(N, heads, Tq, Tk):
    return N * heads * (32 * math.ceil(Tq / 32)) * (32 * math.ceil(Tk / 32))


def test_header_export_table_and_ctypes_table_agree_on_the_new_symbols():
    from ytvln import _lib
    lib = _lib.load()
    decls = header_decls()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in exported.splitlines() if " T " in ln}
    for name in NEW:
        assert name.startswith("ytvln_attn_")          # (the benchmark's attention family timer goes by this prefix)
        assert name in decls and name in exported and hasattr(lib, name), name
        assert _lib.SIGNATURES[name] == [ctype_of(a) for a in decls[name][1]], name
    assert decls["ytvln_attn_bwd_workspace_elems"][0] == "int64_t" and _lib.RESTYPES["ytvln_attn_bwd_workspace_elems"] is _lib.I64
    assert lib.ytvln_version() == 2


def test_default_sets_the_stored_ds_bit():
    import os

    from ytvln import _lib
    if "YTVLN_ATTN_W1" not in os.environ:
        assert _lib.options()["ATTN_W1"] & 8


def test_size_query_counts_whole_blocks(options):
    from ytvln import _lib
    q = _lib.load().ytvln_attn_bwd_workspace_elems
    options(ATTN_W1=15, ATTN_W1_DKV_ANY=0)
    # the training step's sites: image self-attention, the co-attention pair (either order), text self-attention
    assert q(56, 8, 128, 288, 288, 0, 0) == blocks(56, 8, 288, 288) == 56 * 8 * 288 * 288
    assert q(56, 8, 128, 80, 288, 288, 80) == q(56, 8, 128, 288, 80, 80, 288) == 2 * blocks(56, 8, 80, 288) == 2 * 56 * 8 * 96 * 288
    assert q(56, 12, 64, 80, 80, 0, 0) == blocks(56, 12, 80, 80)
    assert q(32, 8, 128, 500, 512, 0, 0) == 32 * 8 * 512 * 512          # the longest sequences
    options(ATTN_W1_DKV_ANY=1)          # ragged tiles, a single score
    assert q(2, 2, 128, 37, 101, 0, 0) == 2 * 2 * 64 * 128
    assert q(2, 2, 128, 37, 101, 101, 37) == 2 * 2 * 2 * 64 * 128
    assert q(1, 1, 64, 1, 1, 0, 0) == 1024


def test_size_query_is_zero_whenever_the_launch_recomputes(options):
    from ytvln import _lib
    q = _lib.load().ytvln_attn_bwd_workspace_elems
    options(ATTN_W1=15, ATTN_W1_DKV_ANY=1)
    assert q(2, 2, 128, 64, 64, 0, 0) > 0
    assert q(2, 2, 96, 64, 64, 0, 0) == 0 and q(2, 2, 68, 64, 64, 0, 0) == 0 and q(2, 2, 32, 64, 64, 0, 0) == 0          # padded heads
    assert q(2, 2, 128, 64, 576, 0, 0) == 0 and q(2, 2, 128, 576, 64, 0, 0) == 0                                          # a sequence past 512
    assert q(2, 2, 128, 64, 64, 64, 576) == 0                                                                              # ... in either problem
    assert q(0, 2, 128, 64, 64, 0, 0) == 0 and q(2, 2, 128, 0, 64, 0, 0) == 0 and q(2, 2, 128, 64, 64, 64, 0) == 0      # nothing to launch
    options(ATTN_W1=7)          # bit 3 cleared
    assert q(56, 8, 128, 288, 288, 0, 0) == 0
    options(ATTN_W1=11)         # the one-wave dK/dV kernel switched off: no wave holds a whole dS block
    assert q(56, 8, 128, 288, 288, 0, 0) == 0
    options(ATTN_W1=15, ATTN_W1_DKV_ANY=0)          # the fill rule sends these launches to the wave-pair dK/dV kernel
    assert q(2, 8, 128, 288, 288, 0, 0) == 0          # 144 waves of 1024 slots
    assert q(28, 8, 128, 288, 288, 0, 0) > 0          # 2016 waves: 98 % of two rounds
    assert q(29, 8, 128, 288, 288, 0, 0) == 0         # 2088 waves: 68 % of three rounds
    assert q(3, 8, 128, 288, 80, 80, 288) == 0


def test_null_problem_is_rejected_without_touching_the_gpu():
    from ytvln import _lib
    lib = _lib.load()
    assert lib.ytvln_attn_bwd_pair_ws(None, None, 1, 1, 128, 0.1, None, None, 0, None) != 0
    assert b"null problem" in lib.ytvln_last_error()
