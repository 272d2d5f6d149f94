"""fastmax_hip_plan against tests/plan_cases.py: every case names the kernels the list expects, the list covers every
(kernel, dtype), (scan, split) and (layout variant, kernel) the dispatch grid of tools/dispatch_table.py can reach, both sides
of every threshold are there and differ, and the inputs the GPU test will use keep the denominator away from zero.
Host arithmetic only: the addresses are made up and never dereferenced, nothing is launched."""
import ctypes
import os
import sys

import numpy as np
import pytest

import plan_cases as pc
from fastmax_experiments_amd._lib import E_ALIGNMENT, E_BAD_SHAPE, E_NULL, Plan, Problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dispatch_table  # noqa: E402

FWD_OPERAND_LAYOUTS = ("q_off8", "o_off8", "k_rowpad")          # variants that touch an operand of the forward


@pytest.fixture(scope="module")
def L():
    from fastmax_experiments_amd import _lib, build
    build.build()
    return _lib.lib()


def _plan(L, c):
    prob = pc.problem(c)
    with pc.tuned(L, c):
        return pc.query(L, prob, pc.fake_operands(prob, c.layout))


@pytest.mark.parametrize("c", pc.CASES, ids=[c.id for c in pc.CASES])
def test_case_names_the_expected_kernels(L, c):
    rc, plan = _plan(L, c)
    assert rc == plan.rc
    assert pc.answer(plan) == pc.expected(c)
    # the family is the forward kernel's, the kept states belong to a split scan, and both match the older queries
    prob = pc.problem(c)
    ops = pc.fake_operands(prob, c.layout)
    with pc.tuned(L, c):
        assert plan.state_bytes == L.fastmax_hip_forward_state_bytes(ctypes.byref(prob), *ops[:7])
        fwd_only = pc.query(L, prob, ops, forward_only=True)[1]
    assert (plan.state_bytes > 0) == (c.split and c.fwd in pc.SCANS)
    assert (fwd_only.rc, fwd_only.path, fwd_only.fwd_kernel, fwd_only.state_bytes) == (plan.rc, plan.path, plan.fwd_kernel, plan.state_bytes)
    assert fwd_only.bwd_kernel == -1
    if c.layout == "aligned" and c.rc == 0:
        assert plan.path == L.fastmax_hip_select_path(ctypes.byref(prob))
    family = {"FWD_QUADRATIC": 1, "FWD_RECURRENT": 2, "FWD_UNMASKED_LIN": 3, "FWD_QUAD32": 4, "FWD_QUAD_MFMA": 4, None: -1}
    assert plan.path == family.get(c.fwd, 3)


def test_bad_problems_and_missing_operands_are_answered_with_their_code(L):
    c = pc.CASES[0]
    prob = pc.problem(c)
    ops = list(pc.fake_operands(prob, "aligned"))
    plan = Plan()
    assert L.fastmax_hip_plan(ctypes.byref(prob), *ops, None) == E_NULL
    assert L.fastmax_hip_plan(None, *ops, ctypes.byref(plan)) == E_NULL and plan.rc == E_NULL
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11):          # one operand missing; grad_o alone missing is still a backward query
        bad = list(ops)
        bad[i] = None
        assert L.fastmax_hip_plan(ctypes.byref(prob), *bad, ctypes.byref(plan)) == E_NULL, i
        assert (plan.rc, plan.path, plan.fwd_kernel, plan.bwd_kernel) == (E_NULL, -1, -1, -1)
    p3 = pc.problem(c)
    p3.p = 3
    assert L.fastmax_hip_plan(ctypes.byref(p3), *ops, ctypes.byref(plan)) == -1 and plan.fwd_kernel == -1
    forced = pc.problem(c)
    forced.path = 2          # recurrent on p = 2: the forward rejects the call, the backward would still run the tiles
    forced.p = 2
    assert L.fastmax_hip_plan(ctypes.byref(forced), *ops, ctypes.byref(plan)) == E_BAD_SHAPE
    assert (plan.fwd_kernel, plan.bwd_kernel) == (-1, pc._lib.BWD_KERNELS.index("BWD_QUAD_MFMA"))


def _coverage(rows):
    """rows: (layout, in dtype number, (rc, fwd, bwd, split)) -> the four sets the case list has to contain"""
    fwd_dt, bwd_dt, scan_split, lay = set(), set(), set(), set()
    for layout, dt, (rc, fwd, bwd, split) in rows:
        if rc not in (0, E_ALIGNMENT):
            continue          # a forced family that does not apply: no forward, and Python never gets to the backward
        if rc == 0:
            fwd_dt.add((fwd, pc.DTYPE_NAMES[dt]))
            if fwd in pc.SCANS:
                scan_split.add((fwd, split))
        bwd_dt.add((bwd, pc.DTYPE_NAMES[dt]))
        if layout != "aligned":
            # a variant is judged by the kernels of the calls its operand goes to: grad_o and dq never reach the forward
            if layout in FWD_OPERAND_LAYOUTS:
                lay.add((layout, "forward", fwd if rc == 0 else "E_ALIGNMENT"))
            lay.add((layout, "backward", bwd))
    return {"(forward kernel, dtype)": fwd_dt, "(backward kernel, dtype)": bwd_dt, "(scan kernel, split)": scan_split,
            "(layout variant, kernel)": lay}


@pytest.fixture(scope="module")
def reachable(L):
    rows = []
    for key in dispatch_table.problems():
        bh, nq, nk, d, (idt, odt), p, causal, path = key
        b, h = dispatch_table.BH[bh]
        prob = Problem(b, h, nq, nk, d, idt, odt, p, causal, 1.0, 0.5, float(nq), path)
        for layout in pc.LAYOUTS:
            rc, plan = pc.query(L, prob, pc.fake_operands(prob, layout))
            if rc in (0, E_ALIGNMENT):
                rows.append((layout, idt, pc.answer(plan)))
    return _coverage(rows)


def test_the_cases_cover_everything_the_dispatch_grid_reaches(reachable, capsys):
    """computed, not claimed: a kernel, dtype, split or layout route that appears in the sweep without a case fails here"""
    have = _coverage([(c.layout, pc.DTYPES[c.dtype], pc.expected(c)) for c in pc.CASES])
    with capsys.disabled():
        for what, found in reachable.items():
            print(f"\nreachable {what}: {sorted(found, key=str)}")
    assert len(reachable["(forward kernel, dtype)"]) >= 21 and len(reachable["(backward kernel, dtype)"]) >= 17
    assert reachable["(scan kernel, split)"] == {(k, s) for k in pc.SCANS for s in (False, True)}
    for what, found in reachable.items():
        missing = found - have[what]
        assert not missing, f"{what} reachable without a case in tests/plan_cases.py: {sorted(missing, key=str)}"
    # and on the GPU: every kernel of every dtype is launched by a case that runs there
    gpu = _coverage([(c.layout, pc.DTYPES[c.dtype], pc.expected(c)) for c in pc.GPU_CASES])
    for what in ("(forward kernel, dtype)", "(backward kernel, dtype)", "(scan kernel, split)"):
        assert have[what] == gpu[what], (what, have[what] - gpu[what])
    assert reachable["(layout variant, kernel)"] <= gpu["(layout variant, kernel)"]


@pytest.mark.parametrize("what,lo,hi,field", pc.BOUNDARIES, ids=[b[0] for b in pc.BOUNDARIES])
def test_both_sides_of_every_threshold_are_cases_and_differ(L, what, lo, hi, field):
    a, b = pc.BY_ID[lo], pc.BY_ID[hi]
    # one step apart in exactly one size, everything else equal
    diff = [i for i in range(5) if a.shape[i] != b.shape[i]]
    if a.shape[2] == a.shape[3] and b.shape[2] == b.shape[3] and diff == [2, 3]:
        diff = [2]
    assert len(diff) == 1 and a[2:7] == b[2:7] and a.tune == b.tune and a.out == b.out, (a, b)
    i = diff[0]
    assert b.shape[i] - a.shape[i] in ((1,) if i < 4 else (1, 2, 4, 8)), "neighbouring sizes (head sizes: neighbouring multiples)"
    assert getattr(a, field) != getattr(b, field)
    for c in (a, b):
        assert pc.answer(_plan(L, c)[1]) == pc.expected(c)
    # the smaller side runs on the GPU, unless the pair is about head counts or the 20000-token rule (host-only by design)
    assert a.gpu or what.startswith(("B*H", "N 20000")), a.id


def test_gpu_cases_stay_small():
    for c in pc.GPU_CASES:
        B, H, Nq, Nk, D = c.shape
        assert B * H <= 8 and max(Nq, Nk) <= 520, c.id          # 8 heads: the per-XCD workgroup mapping of the 32-row tiles
    assert len({c.id for c in pc.CASES}) == len(pc.CASES)


def _one_case_per_problem():
    seen = {}
    for c in pc.GPU_CASES:
        seen.setdefault((c.shape, c.dtype, c.mask, c.p), c)
    return list(seen.values())


@pytest.mark.parametrize("c", _one_case_per_problem(), ids=lambda c: c.id)
def test_the_denominator_of_every_gpu_case_is_well_conditioned(c):
    """g = Nq + a q . ksum (unmasked) must stay above a quarter of its constant, and the masked g above 0.25 in every row (row 0
    is 1 + a q0 . k0 for p = 1): then the GPU test can hold these cases to the suite's ordinary tolerances.  The layout variants
    and forced paths of a problem use the same tensors, so one check per problem is enough."""
    g = pc.oracle_fwd(c)[1]
    floor = 0.25 if c.mask else 0.25 * c.shape[2]
    assert float(np.abs(g).min()) >= floor, float(np.abs(g).min())
    if c.mask:
        assert float(np.abs(g[:, :, 0]).min()) >= 0.25
