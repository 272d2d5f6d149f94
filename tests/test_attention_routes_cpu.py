"""Which route a linearmax call and the attention sub-layer take, pinned row by row: tests/golden/attention_routes.json holds
what RAN on an MI355X before fastmax_hack.linearmax_plan and CausalSelfAttention.plan existed (tools/attention_routes.py
--record), and the plans have to give those answers.  Host arithmetic only: the library is built, no device is needed."""
import ctypes
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import attention_routes  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    from fastmax_experiments_amd import build
    build.build()
    with open(attention_routes.GOLDEN) as f:
        return json.load(f)


def test_plans_answer_as_recorded(golden):
    assert [g["args"] for g in golden] == attention_routes.rows() and len(golden) > 300
    bad = [(g["args"], g["plan"], attention_routes.answer(g["args"])) for g in golden if attention_routes.answer(g["args"]) != g["plan"]]
    assert not bad, f"{len(bad)} rows differ, first (arguments, recorded, now): {bad[0]}"


def test_route_rows_reach_every_answer(golden):
    ops_ = [g["plan"] for g in golden if g["args"]["kind"] == "op"]
    blocks = [g["plan"] for g in golden if g["args"]["kind"] == "block"]
    in_blocks = [p["operator"] for p in blocks if p["operator"] != "fastmax"]
    for plans in (ops_, in_blocks):
        assert {p.get("operator") for p in plans} - {None} == {"fused_forward", "one_node", "two_node", "unmasked"}
        assert {p.get("prologue") for p in plans} - {None} == {"in_scan", "cast"}
        assert {p.get("prologue_bwd") for p in plans} - {None} == {"both", "q", "none"}
        assert {p.get("k_layout") for p in plans} - {None} == {"per_head", "group_copies", "group_views"}
    assert {p.get("slices") for p in ops_} == {1, 2, None}
    assert {p.get("raises") for p in ops_} == {"NotImplementedError", None}
    assert {p["qkv"] for p in blocks} == {"gemm_epilogue", "hip_pass", "eager"}
    assert {p["kv_layout"] for p in blocks} == {0, 1, 2, 3, 4}
    assert "fastmax" in [p["operator"] for p in blocks]


def test_forward_only_coverage_is_the_library_s(golden):
    """the plan's rule for the forward-only fused kernel (D <= 128 in whole 16-byte pieces, the heads of a slice fit a launch)
    against fastmax_hip_linearmax_forward_auto itself: aligned dummy addresses and no workspace, so a covered problem is
    answered E_WORKSPACE and one linearmax_fwd_check rejects E_BAD_SHAPE; nothing is launched"""
    from fastmax_experiments_amd import _lib
    from fastmax_experiments_amd.attention_mechanisms.fastmax import MAX_HEADS_PER_LAUNCH
    from fastmax_experiments_amd.attention_mechanisms.fastmax_hack import linearmax_plan
    L = _lib.lib()
    seen = set()
    for row in (g["args"] for g in golden if g["args"]["kind"] == "op"):
        dtype = attention_routes._dtype(row["dtype"])
        B, H, N, D = row["B"], row["H"], row["N"], row["D"]
        try:
            covered = linearmax_plan(dtype, B, H, N, N, D, 1, True, False).operator == "fused_forward"
        except NotImplementedError:
            covered = False
        if B * H > MAX_HEADS_PER_LAUNCH:
            B = MAX_HEADS_PER_LAUNCH // H                              # what one slice launches
        dt = {torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}.get(dtype, _lib.F32)
        prob = _lib.Problem(B, H, N, N, D, dt, dt, 1, 1, 1.0, 0.5, 0.0, _lib.PATH_AUTO)
        st = (ctypes.c_int64 * 3)(H * N * D, N * D, D)
        rc = L.fastmax_hip_linearmax_forward_auto(ctypes.byref(prob), 256, st, 256, st, 256, st, 256, 256, None, None, 256, None,
                                                  None, 0, None)
        assert rc == (_lib.E_WORKSPACE if covered else _lib.E_BAD_SHAPE), (row, covered, rc)
        seen.add(covered)
    assert seen == {True, False}
