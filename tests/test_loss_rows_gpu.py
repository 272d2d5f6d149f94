"""The cross-entropy row kernels (csrc/fastmax_ce.hip) entry by entry on an MI355X: per-row loss and lse and every entry of
d(logits) within the allowances of ce_ref.py around its float64 reference, on the shared case table (every dtype; row lengths
around the 16-byte piece and the 256-thread sweep; contiguous, 16-byte rows with a ragged last piece, a base pointer off the
16-byte grid, an output stride of its own, in place; shifted, wide, equal, peaked, masked (-inf) and extreme logits; every kind
of unscored row; a per-row gradient with a scale).  Beside the numbers: exact zeros where the contract says zero, nothing
written outside [0, V) of any row, and the same bits from every layout and from a second call.  Then the same allowances
through cross_entropy_rows and chunked_cross_entropy.

Observed on an MI355X (worst error / allowance over the table, an observation, not a bound):
  direct calls, 1881 cases   f32: loss 0.209  lse 0.164  dz 0.396;   bf16: loss 0.130  lse 0.160  dz 0.994;
                             f16: loss 0.160  lse 0.158  dz 0.927   (16-bit dz: half-ulp rounding nearly attains u by itself)
  cross_entropy_rows         f32 0.185, bf16 0.954, f16 0.893;   chunked_cross_entropy d(logits): f32 0.238, bf16 0.993
A row loss formed as (m + log s) - z_t is 1.45x to 7.84x over b_loss on the +1000 cases and 437x on the fp16 extremes."""
import itertools

import numpy as np
import pytest
import torch

import ce_ref as cr

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0                       # finite in every dtype, and far above every logit of the table but the fp16 extremes
INT = {"f32": torch.int32, "bf16": torch.int16, "f16": torch.int16}
GROUPS = {k: list(v) for k, v in itertools.groupby(sorted(cr.CASES, key=lambda c: (c.dt, c.V, c.M)), key=lambda c: (c.dt, c.V, c.M))}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from fastmax_experiments_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _guarded(M, V, ld, dt, lead=0):
    """-> (flat, view): `view` is the (M, V) column slice of rows 1..M of an (M + 2, ld) buffer that starts `lead` elements into
    an aligned allocation; everything is pre-filled with the sentinel"""
    assert ld >= V and lead >= 0
    flat = torch.full((lead + (M + 2) * ld,), SENTINEL, dtype=cr.TD[dt], device="cuda")
    return flat, flat[lead:].view(M + 2, ld)[1:M + 1, :V]


def _bits(x, dt=None):
    return x.contiguous().view(torch.int32 if dt is None else INT[dt])


def _up(V, E):
    return (V + E - 1) // E * E


def _run(c, inp, z_dev, t_dev, g_dev):
    """one forward and one backward call in the case's layout -> (loss, lse, dz as a contiguous copy); checks on the way that
    nothing outside [0, V) of the rows of either buffer changed"""
    from fastmax_experiments_amd.loss import _rows_backward, _rows_forward
    dt, M, V = c.dt, c.M, c.V
    E = cr.piece(dt)
    ld = V if c.layout in ("contig", "offset") else _up(V, E)
    zflat, z = _guarded(M, V, ld, dt, lead=1 if c.layout == "offset" else 0)
    z.copy_(z_dev)
    if c.layout == "ragged":
        assert z.data_ptr() % 16 == 0 and (z.stride(0) * z.element_size()) % 16 == 0 and V % E != 0        # the vector path
    if c.layout == "offset":
        assert z.data_ptr() % 16 == z.element_size() and V % E == 0
    if c.layout == "inplace":
        oflat, out = zflat, z
    else:
        oflat, out = _guarded(M, V, ld + 2 * E if c.layout == "outstride" else ld, dt)
    assert c.layout != "outstride" or out.stride(0) != z.stride(0)
    z_before = zflat.clone()
    loss, lse = _rows_forward(z, t_dev, inp.ignore_index)
    assert torch.equal(_bits(zflat, dt), _bits(z_before, dt)), "the forward pass wrote to the logits"
    want = oflat.clone()
    _rows_backward(z, t_dev, lse, g_dev, inp.grad_scale, inp.ignore_index, out)
    dz = out.clone()
    want.view(M + 2, -1)[1:M + 1, :V].copy_(out)            # the output buffers start at their allocation
    assert torch.equal(_bits(oflat, dt), _bits(want, dt)), "the backward pass wrote outside [0, V) of its rows"
    if c.layout != "inplace":
        assert torch.equal(_bits(zflat, dt), _bits(z_before, dt)), "the backward pass wrote to the logits"
    return loss, lse, dz


@pytest.mark.parametrize("dt,V,M", sorted(GROUPS), ids=lambda v: str(v))
def test_rows_kernels_entry_by_entry(dt, V, M):
    failures, worst = [], {"loss": 0.0, "lse": 0.0, "dz": 0.0}
    shared = {}
    for c in GROUPS[(dt, V, M)]:
        key = cr.numeric_key(c)
        if key not in shared:
            assert c.layout == "contig"                     # the table lists the contiguous layout first
            inp = cr.case_inputs(c)
            shared[key] = dict(inp=inp, ref=cr.ce_rows_ref(inp.z, inp.t, inp.ignore_index, inp.g),
                               bounds=cr.ce_bounds(inp.z, inp.t, inp.g, dt, inp.ignore_index),
                               z=torch.from_numpy(inp.z).to(cr.TD[dt]).cuda(), t=torch.from_numpy(inp.t).cuda(),
                               g=None if inp.grad_rows is None else torch.from_numpy(inp.grad_rows).cuda())
        s = shared[key]
        inp = s["inp"]
        loss, lse, dz = _run(c, inp, s["z"], s["t"], s["g"])
        again = _run(c, inp, s["z"], s["t"], s["g"])
        r = cr.worst_ratios(inp.z, inp.t, loss.cpu().numpy(), lse.cpu().numpy(), dz.double().cpu().numpy(), s["ref"], s["bounds"],
                            inp.ignore_index)
        print(f"{c}: error/allowance loss {r['loss']:.3f} lse {r['lse']:.3f} dz {r['dz']:.3f}")
        worst = {k: max(worst[k], r[k]) for k in worst}
        bad = [f"{k} {v:.3g}x its allowance" for k, v in r.items() if not v <= 1.0]
        got = (_bits(loss), _bits(lse), _bits(dz, dt))
        if not all(torch.equal(a, b) for a, b in zip(got, (_bits(again[0]), _bits(again[1]), _bits(again[2], dt)))):
            bad.append("a second call gave other bits")
        if c.layout == "contig":
            s["bits"] = got
        elif not all(torch.equal(a, b) for a, b in zip(got, s["bits"])):
            bad.append("other bits than the contiguous layout")
        if bad:
            failures.append(f"{c}: " + "; ".join(bad))
    print(f"WORST {dt} V={V}: loss {worst['loss']:.3f} lse {worst['lse']:.3f} dz {worst['dz']:.3f}")
    assert not failures, f"{len(failures)} of {len(GROUPS[(dt, V, M)])} cases:\n" + "\n".join(failures[:40])


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_cross_entropy_rows_returns_the_row_losses_in_the_logits_dtype(dt):
    """the float32 row loss within b_loss, then one rounding to the logits' dtype: u |loss| + b_loss"""
    from fastmax_experiments_amd.loss import cross_entropy_rows
    failures, worst = [], 0.0
    for c in cr.CASES:
        if c.dt != dt or c.layout != "contig" or c.grad != "none":
            continue
        inp = cr.case_inputs(c)
        loss, _, _, _ = cr.ce_rows_ref(inp.z, inp.t, inp.ignore_index, inp.g)
        b = cr.UNIT[dt] * np.abs(loss) + cr.ce_bounds(inp.z, inp.t, inp.g, dt, inp.ignore_index).b_loss
        got = cross_entropy_rows(torch.from_numpy(inp.z).to(cr.TD[dt]).cuda(), torch.from_numpy(inp.t).cuda(), inp.ignore_index)
        assert got.dtype == cr.TD[dt] and got.shape == (c.M,)
        got = got.double().cpu().numpy()
        ok = cr.scored(inp.t, c.V, inp.ignore_index)
        r = float((np.abs(got - loss) / b).max()) if np.isfinite(got).all() and (got[~ok] == 0).all() else float("inf")
        worst = max(worst, r)
        if not r <= 1.0:
            failures.append(f"{c}: {r:.3g}x the allowance")
    print(f"cross_entropy_rows {dt}: worst error/allowance {worst:.3f}")
    assert not failures, "\n".join(failures[:40])


@pytest.mark.parametrize("dt,tol", [("f32", None), ("bf16", 6e-3)])
def test_chunked_cross_entropy_on_a_short_last_chunk(dt, tol):
    """a list of lm-head chunks whose last one is shorter (T = 300 by 128).  600 rows, 512 of them scored: the mean's 1 / n is
    then exact in every dtype, so d(total)/d(row loss) is 1 / n as it stands (the wrapper's row losses, and with them their
    gradients, are in the logits' dtype: for another n the 16-bit g is 1 / n rounded to it).  The gradient meets b_dz entry by
    entry.  The float32 value: every row within b_loss, and the float32 sum of 600 rows and the division add at most
    16 * 2^-24 |mean| (a reduction tree of 10 levels, the concatenation's copies exact); the 16-bit value within the tolerance
    test_loss_gpu.py has for it."""
    from fastmax_experiments_amd.loss import chunked_cross_entropy
    E = cr.piece(dt)
    B, T, V = 2, 300, 2 * 256 * E + E + 3
    rng = np.random.default_rng(V)
    z = cr.round_to(rng.standard_normal((B * T, V)) * 3, dt)
    t = rng.integers(0, V, size=B * T)
    off = rng.permutation(B * T)[:88]
    t[off[:80]], t[off[80:84]], t[off[84:]] = -1, -100, V + 7
    first = np.flatnonzero(cr.scored(t, V, -1))[:2]
    t[first[0]], t[first[1]] = V - 1, 0
    n = int(cr.scored(t, V, -1).sum())
    assert n == 512
    g = np.full(B * T, 1.0 / n)
    ref = cr.ce_rows_ref(z, t, -1, g)
    bounds = cr.ce_bounds(z, t, g, dt, -1)
    mean = ref[0].sum() / n
    x = torch.from_numpy(z).to(cr.TD[dt]).view(B, T, V).cuda().requires_grad_(True)
    targets = torch.from_numpy(t).view(B, T).cuda()
    chunks = list(x.split(128, dim=1))
    assert [ch.size(1) for ch in chunks] == [128, 128, 44]
    value = chunked_cross_entropy(chunks, targets, chunk_size=128, ignore_index=-1)
    value.backward()
    value = value.detach()
    assert value.dtype == cr.TD[dt] and x.grad.dtype == cr.TD[dt]
    if tol is None:
        allowed = float(bounds.b_loss[cr.scored(t, V, -1)].mean() + 16 * 2.0 ** -24 * abs(mean))
    else:
        allowed = tol * max(1.0, abs(mean))
    print(f"chunked {dt}: value {float(value):.8f} float64 {mean:.8f} |difference| {abs(float(value) - mean):.3e} allowed {allowed:.3e}")
    assert abs(float(value) - mean) <= allowed
    dz = x.grad.view(B * T, V).double().cpu().numpy()
    r = cr.worst_ratios(z, t, ref[0], ref[1], dz, ref, bounds, -1)["dz"]
    print(f"chunked {dt}: gradient worst error/allowance {r:.3f}")
    assert r <= 1.0
