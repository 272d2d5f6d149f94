"""What the host side of the library decides, pinned row by row: tests/golden/dispatch_table.json was recorded by
tools/dispatch_table.py from the library as it was before path selection moved into the plan functions of
csrc/fastmax_api.hip, and every answer has to stay what it was: selected path, workspace sizes, kept-state bytes,
linearmax-train coverage, and the return code of every call that is rejected before a launch.  Host arithmetic only."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dispatch_table  # noqa: E402


@pytest.fixture(scope="module")
def tables():
    from fastmax_experiments_amd import build
    build.build()
    with open(dispatch_table.GOLDEN) as f:
        return json.load(f), dispatch_table.table()


def test_every_case_answers_as_recorded(tables):
    golden, now = tables
    assert golden["columns"] == now["columns"]
    assert len(golden["cases"]) == len(now["cases"]) > 4000
    bad = [(g, n) for g, n in zip(golden["cases"], now["cases"]) if g != n]
    assert not bad, f"{len(bad)} rows differ, first (recorded, now): {bad[0]}"


def test_every_rejected_call_returns_the_recorded_code(tables):
    golden, now = tables
    assert len(golden["rejected"]) == len(now["rejected"]) > 300
    bad = [(g, n) for g, n in zip(golden["rejected"], now["rejected"]) if g != n]
    assert not bad, f"{len(bad)} calls differ, first (recorded, now): {bad[0]}"


def test_the_table_reaches_every_branch_of_path_selection(tables):
    """the thinned grid still sees every family, every rejection of a forced path, the sequence split with and without
    kept states, and a layout that loses them"""
    golden, _ = tables
    col = {c: i for i, c in enumerate(golden["columns"])}
    rows = golden["cases"]
    for forced in range(5):
        got = {r[col["select_path"]] for r in rows if r[col["path"]] == forced}
        assert (got >= {1, 2, 3, 4, -2}) if forced == 0 else (-2 in got and forced in got), (forced, got)
    kept = [r for r in rows if r[col["state_bytes"]] > 0]
    assert kept and all(r[col["state_bytes"]] == r[col["forward_workspace"]] for r in kept)
    assert all(r[col[c]] == 0 for r in kept for c in ("state_bytes_q_plus_8", "state_bytes_k_stride_plus_8", "state_bytes_o_plus_8"))
    assert any(r[col["forward_workspace"]] > 0 and r[col["causal"]] == 0 for r in rows)            # unmasked linear
    assert {r[col["D"]] for r in kept} >= {8, 64, 72, 128}
    assert {r[2] for r in golden["rejected"] if r[0].startswith("fastmax_hip_linearmax") or r[0].endswith(("forward", "states"))} >= {-1, -2, -3, -4, -5, -6}
