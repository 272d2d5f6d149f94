"""The cross-entropy reference and its allowances (ce_ref.py), proven without a GPU: the reference against torch's float64
cross_entropy and autograd; the allowances against a float32 emulation of the kernel's documented arithmetic (they can be met,
with room) and against mutants of that emulation (each is rejected); and the tensor-scale metric the older loss tests use
against the first mutant (it is accepted -- why the per-entry bounds exist)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ce_ref as cr
from conftest import rel_err

NUMERIC = sorted({cr.numeric_key(c) for c in cr.CASES})
DTYPES = ("f32", "bf16", "f16")


@functools.lru_cache(maxsize=None)
def _setup(key):
    c = cr.Case(key[0], key[1], key[2], "contig", key[3], key[4])
    inp = cr.case_inputs(c)
    ref = cr.ce_rows_ref(inp.z, inp.t, inp.ignore_index, inp.g)
    return c, inp, ref, cr.ce_bounds(inp.z, inp.t, inp.g, c.dt, inp.ignore_index)


def emulate(inp, dt, mutant=None):
    """the kernel's arithmetic in float32: max, exp(x - m) summed, lse = m + log s, loss = log s + (m - z_t), p = exp(x - lse),
    times g, one rounding to the dtype.  `mutant` names one deliberate mistake."""
    f32 = np.float32
    x = inp.z.astype(f32)
    M, V = x.shape
    E = cr.piece(dt)
    ok = cr.scored(inp.t, V, inp.ignore_index)
    tt = np.where(ok, inp.t, 0)
    rows = np.arange(M)
    m = x.max(1)
    with np.errstate(under="ignore"):
        e = np.exp(x - m[:, None])
    if mutant == "last_entry":
        e[:, V - 1] = 0
    if mutant == "wave":                                   # wave 1's pieces never reach the sum
        e[:, ((np.arange(V) // E) % 256) // 64 == 1] = 0
    s = e.sum(1, dtype=f32)
    with np.errstate(divide="ignore"):                     # a mutant may leave nothing in the sum
        ls = np.log(s)
    lse = (m + ls).astype(f32)
    zt = x[rows, tt]
    loss = (lse - zt) if mutant == "old_loss" else ls + (m - zt)
    loss = np.where(ok, loss, f32(0)).astype(f32)
    if mutant == "unscored_loss":
        loss = np.where(ok, loss, f32(1e-3))
    with np.errstate(under="ignore"):
        p = np.exp(x - lse[:, None])
    onehot = np.zeros_like(x)
    onehot[rows[ok], tt[ok]] = 1
    g = np.ones(M, f32) if inp.grad_rows is None else inp.grad_rows * f32(inp.grad_scale)
    if mutant == "row_scale":
        g = np.roll(g, 1)
    g = np.where(ok, g, f32(0)).astype(f32)
    if mutant == "small_p":
        p = np.where((p < 1e-3) & (onehot == 0), f32(0), p)
    if mutant == "last_entry":
        p[:, V - 1] = 0
    with np.errstate(invalid="ignore"):
        d = ((p - onehot) * g[:, None]).astype(f32)
    if mutant == "scaled":
        d = d * f32(1 + (2e-5 if dt == "f32" else 3 * cr.UNIT[dt]))
    return loss.astype(np.float64), lse.astype(np.float64), cr.round_to(d, dt)


def _ratios(key, mutant=None):
    c, inp, ref, bounds = _setup(key)
    loss, lse, dz = emulate(inp, c.dt, mutant)
    return cr.worst_ratios(inp.z, inp.t, loss, lse, dz, ref, bounds, inp.ignore_index)


def test_case_table_covers_what_it_promises():
    for dt in DTYPES:
        E = cr.piece(dt)
        mine = [c for c in cr.CASES if c.dt == dt and c.M == 5]
        assert {c.V for c in mine} == {1, 2, E - 1, E, E + 1, 256 * E - 1, 256 * E, 256 * E + 1, 2 * 256 * E + E + 3, 4099}
        assert {c.layout for c in mine} == set(cr.LAYOUTS) and {c.grad for c in mine} == set(cr.GRADS)
        assert {c.values for c in mine} == set(cr.VALUES) - (set() if dt == "f16" else {"f16_extremes"})
        assert all(c.V % E != 0 for c in mine if c.layout == "ragged") and all(c.V % E == 0 for c in mine if c.layout == "offset")
        kinds = set()
        for key in NUMERIC:
            if key[0] != dt:
                continue
            c, inp, ref, _ = _setup(key)
            ok = cr.scored(inp.t, c.V, inp.ignore_index)
            kinds |= {"ignore" if t == inp.ignore_index else "negative" if t < 0 else "beyond" for t in inp.t[~ok]}
            assert np.isfinite(inp.z[np.arange(c.M)[ok], inp.t[ok]]).all()          # no target is masked
            assert inp.t[1] == 0 and (c.values == "masked" or inp.t[0] == c.V - 1)
            assert np.array_equal(cr.round_to(inp.z, dt), inp.z)
            if c.values == "masked":
                assert np.isneginf(inp.z[:, cr.mask_start(dt, c.V):]).all() and np.isneginf(inp.z).sum(1).min() >= 2 * E + 6
            if inp.grad_rows is not None:
                assert (inp.grad_rows[ok] == 0).any() and (inp.grad_rows[ok] < 0).any()
        assert kinds == {"ignore", "negative", "beyond"}
    big = [c for c in cr.CASES if c.V == 32000]
    assert len(big) == 1 and big[0].dt == "bf16" and big[0].M == 8


@pytest.mark.parametrize("dt", DTYPES)
def test_reference_matches_torch_float64(dt):
    worst = 0.0
    for key in NUMERIC:
        if key[0] != dt:
            continue
        c, inp, (loss, lse, p, dz), _ = _setup(key)
        ok = cr.scored(inp.t, c.V, inp.ignore_index)
        z = torch.from_numpy(inp.z[ok]).requires_grad_(True)
        rows = F.cross_entropy(z, torch.from_numpy(inp.t[ok]), reduction="none")
        (rows * torch.from_numpy(inp.g[ok])).sum().backward()
        # 1e-12 of max(1, |value|): float64 numbers near the fp16 extremes (6e4) are themselves 7e-12 apart
        worst = max(worst, float((np.abs(rows.detach().numpy() - loss[ok]) / np.maximum(1, np.abs(loss[ok]))).max()),
                    float(np.abs(z.grad.numpy() - dz[ok]).max()),
                    float((np.abs(torch.logsumexp(torch.from_numpy(inp.z), 1).numpy() - lse) / np.maximum(1, np.abs(lse))).max()))
        assert (loss[~ok] == 0).all() and (dz[~ok] == 0).all() and np.isfinite(lse).all()
        assert np.allclose(p.sum(1), 1.0, rtol=0, atol=1e-10)          # lse near 6e4 is known to 7e-12
    print(f"reference against torch float64, {dt}: worst difference {worst:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("dt", DTYPES)
def test_the_bounds_can_be_met(dt):
    """error / allowance of the float32 emulation: at most 0.5 for the float32 quantities, below 1 for 16-bit dz (half-ulp
    rounding nearly attains u, so that figure is close to 1 by construction)"""
    worst = {"loss": 0.0, "lse": 0.0, "dz": 0.0}
    for key in NUMERIC:
        if key[0] == dt:
            r = _ratios(key)
            worst = {k: max(worst[k], r[k]) for k in worst}
    print(f"emulation, {dt}: worst error/allowance loss {worst['loss']:.3f} lse {worst['lse']:.3f} dz {worst['dz']:.3f}")
    assert worst["loss"] <= 0.5 and worst["lse"] <= 0.5
    assert worst["dz"] <= 0.5 if dt == "f32" else worst["dz"] < 1.0


MUTANTS = ("small_p", "last_entry", "wave", "row_scale", "scaled", "unscored_loss", "old_loss")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("mutant", MUTANTS)
def test_the_bounds_reject_mutants(mutant, dt):
    worst, where, caught, n = 0.0, None, 0, 0
    for key in NUMERIC:
        if key[0] != dt or (mutant == "old_loss" and key[3] != "plus1000"):
            continue
        r = max(_ratios(key, mutant).values())
        n, caught = n + 1, caught + (r > 1.0)
        if np.isfinite(r) and r > worst:
            worst, where = r, key
    print(f"mutant {mutant}, {dt}: rejected on {caught} of {n} cases; worst finite error/allowance {worst:.3g} at {where}")
    assert caught >= 1


@pytest.mark.parametrize("V", [4099, 32000])
def test_the_old_metric_accepts_the_first_mutant(V):
    """max |dz - ref| / max |ref| < 1e-2, the 16-bit gradient check of test_loss_gpu.py, passes a backward pass that writes zero
    to every non-target entry with p < 1e-3 -- nearly the whole row at V = 32000 -- while the per-entry bound is far exceeded"""
    key = next(k for k in NUMERIC if k[0] == "bf16" and k[2] == V and k[3] == "randn3" and k[4] == "rows")
    c, inp, ref, bounds = _setup(key)
    loss, lse, dz = emulate(inp, c.dt, "small_p")
    zeroed = float((dz[ref[3] != 0] == 0).mean())
    old = rel_err(dz, ref[3])
    new = cr.worst_ratios(inp.z, inp.t, loss, lse, dz, ref, bounds, inp.ignore_index)["dz"]
    print(f"V={V}: {zeroed:.1%} of the nonzero gradient entries zeroed; old metric {old:.2e} (< 1e-2), per-entry error/allowance {new:.0f}")
    assert old < 1e-2 and new > 100
