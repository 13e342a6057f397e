"""Deterministic mode, host side (no GPU): the switch, the environment variable, the workspace sizing helpers, the argument checks
of the workspace entry points and the inverted index of the embedding backward."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import mammo_clip_amd  # noqa: F401
from mammo_clip_amd import ops
import mammo_clip_amd.lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_set_deterministic_round_trips():
    first = ops.deterministic()
    assert ops.set_deterministic(True) == first and ops.deterministic() is True
    assert ops.set_deterministic(False) is True and ops.deterministic() is False
    assert ops.set_deterministic(first) is False and ops.deterministic() == first


@pytest.mark.parametrize("value,expect", [("1", "True"), ("0", "False"), (None, "False")])
def test_environment_switch(value, expect):
    env = {k: v for k, v in os.environ.items() if k != "MC_DETERMINISTIC"}
    if value is not None:
        env["MC_DETERMINISTIC"] = value
    out = subprocess.run([sys.executable, "-c", "import mammo_clip_amd.ops as o; print(o.deterministic())"], cwd=ROOT, env=env,
                         capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split()[-1] == expect, (out.stdout, out.stderr[-500:])


def test_sizing_helpers_answer_without_a_gpu():
    lib = L.load()
    old = lib.mc_dwconv_set_lane_mode(1)
    try:
        a = ops._dw_args(2, 70, 300, 48, 3, 1, 1, 1, 70, 300)
        lane = lib.mc_dwconv_bwd_weight_dw_rows(C.byref(a))
        lib.mc_dwconv_set_lane_mode(0)
        march = lib.mc_dwconv_bwd_weight_dw_rows(C.byref(a))
        assert lane >= 2 and march >= 2 and lane != march          # the kernel form changes with the lane mode, and so does the answer
        assert lib.mc_dwconv_bwd_weight_dw_rows(C.byref(a)) == march
        f = ops._dw_args(2, 70, 300, 48, 3, 1, 1, 1, 70, 300)
        f.epi_x = 16
        assert lib.mc_dwconv_bwd_fused_dw_rows(C.byref(f)) == lib.mc_dwconv_bwd_fused_stat_rows(C.byref(f)) >= 2
        s = ops._dw_args(5, 38, 22, 384, 3, 2, 0, 1, 19, 11)
        s.epi_x, s.xw, s.cin = 16, 16, 64
        assert lib.mc_dwconv_bwd_data_dw_rows(C.byref(s)) == lib.mc_dwconv_bwd_data_stat_rows(C.byref(s)) >= 2
    finally:
        lib.mc_dwconv_set_lane_mode(old)
    assert [lib.mc_add_ln_bwd_ws_rows(r) for r in (1, 4, 5, 2047, 2051, 1 << 20)] == [1, 1, 2, 512, 512, 512]
    plan = (C.c_int * 2)()
    assert lib.mc_bert_embed_bwd_ws_floats(3, 17, 768, 51, plan) == (51 + 3 * 17 + 4 * 13) * 768 and list(plan) == [3, 13]
    assert lib.mc_bert_embed_bwd_ws_floats(64, 256, 768, 64 * 256, plan) == (64 * 256 + 8 * 256 + 4 * 512) * 768 and list(plan) == [8, 512]
    assert lib.mc_bert_embed_bwd_ws_floats(0, 17, 768, 51, None) == 0


def test_workspace_entry_points_refuse_null_pointers():
    lib = L.load()
    assert lib.mc_ordered_sum(None, 2, 8, 8, None, 0, None) != 0 and b"ordered_sum" in lib.mc_last_error()
    assert lib.mc_ordered_sum(16, 0, 8, 8, 16, 0, None) != 0 and b"ordered_sum" in lib.mc_last_error()
    assert lib.mc_add_ln_bwd_ws(*([None] * 6), 8, 768, 0.0, 0, 0, None, None, None, None, None, 2, None) != 0
    assert b"add_ln_bwd_ws: null" in lib.mc_last_error()
    assert lib.mc_add_ln_rows_bwd_ws(*([None] * 7), 8, 768, 0.0, 0, 0, None, None, None, None, None, 2, None) != 0
    assert b"add_ln_rows_bwd_ws: null" in lib.mc_last_error()
    assert lib.mc_bert_embed_bwd_ws(*([None] * 9), 3, 17, 768, 0.0, 0, 0, *([None] * 8), 0, None) != 0
    assert b"embed_bwd_ws: null" in lib.mc_last_error()
    assert lib.mc_bert_embed_rows_bwd_ws(*([None] * 10), 3, 17, 24, 768, 27, 0.0, 0, 0, *([None] * 8), 0, None) != 0
    assert b"embed_rows_bwd_ws: null" in lib.mc_last_error()


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="dummy pointers: the same refusal runs on real buffers in test_deterministic_gpu.py")
def test_weight_gradient_workspace_of_another_form_is_refused():
    """a weight-gradient workspace sized for another kernel form is refused with a status, before any launch"""
    lib = L.load()
    a = ops._dw_args(2, 70, 300, 48, 3, 1, 1, 1, 70, 300)
    a.x = a.dy = a.out = a.dw_partials = 16
    a.dw_rows = lib.mc_dwconv_bwd_weight_dw_rows(C.byref(a)) + 1
    assert lib.mc_dwconv_bwd_weight(C.byref(a), None) != 0 and b"dw_partials" in lib.mc_last_error()


@pytest.mark.parametrize("ids", [[], [7] * 9, list(range(12, 0, -1)), [3, 0, 3, 5, 0, 0, 3]])
def test_inverted_index_against_a_python_loop(ids):
    t = torch.tensor(ids, dtype=torch.int64)
    sorted_ids, order = ops.token_rows_by_id(t)
    want = {}
    for row, i in enumerate(ids):
        want.setdefault(i, []).append(row)
    exp_ids = [i for i in sorted(want) for _ in want[i]]
    exp_rows = [r for i in sorted(want) for r in want[i]]
    assert sorted_ids.tolist() == exp_ids and order.tolist() == exp_rows
    assert sorted_ids.dtype == torch.int64 and order.dtype == torch.int64 and sorted_ids.is_contiguous() and order.is_contiguous()
