"""optim.FlatAdamW (include/fastmax_hip_optim.h, csrc/flat_adamw.hip), everything that needs no device:

1. the size queries, which need no device (the binding table against this header: test_binding_cpu);
2. every rejection the header lists, returned before any launch;
3. the chunk table: every flat index exactly once, no chunk across a segment boundary;
4. the host contract of FlatAdamW: ValueErrors, a state_dict round trip that continues bit for bit;
5. the CPU rehearsal path against the float64 restatement (flat_adamw_ref.py)."""

import numpy as np
import pytest
import torch

from flat_adamw_ref import PARITY_TOL, AdamWRef
from fastmax_experiments_amd import _lib, dp, optim

SIZES = [1, 7, 64, 1023, 1025, 4099]


# ---- 1. size queries (the binding itself: test_binding_cpu) -------------------------------------------------------------------
def test_size_queries_need_no_device():
    L = _lib.lib()
    chunk = L.fastmax_hip_adamw_chunk()
    assert chunk == optim.chunk_elems() and chunk > 0 and chunk % 4 == 0
    assert L.fastmax_hip_adamw_workspace(0) == 0 and L.fastmax_hip_adamw_workspace(-5) == 0
    # the 64-byte scalar record, 64 ticket counters 64 bytes apart, then one float per tile of 4096 elements, at most 1024 of
    # them, padded to 16 bytes
    assert L.fastmax_hip_adamw_workspace(1) == 64 + 4096 + 16
    assert L.fastmax_hip_adamw_workspace(5 * 4096 + 1) == 64 + 4096 + 32
    assert L.fastmax_hip_adamw_workspace(1 << 40) == 64 + 4096 + 4096


# ---- 2. rejections -----------------------------------------------------------------------------------------------------------
A = 0x10000          # a made-up address, 16-byte aligned: every call below is refused before anything could touch it


def _update(**over):
    n = over.pop("n", 5000)
    a = dict(g=A, g_dtype=_lib.F32, n=n, m=A, v=A, master=A, n_lowp=1, segments=A, n_segments=2, chunks=A, n_chunks=6,
             lr=1e-3, lr_ptr=None, beta1=0.9, beta2=0.999, omb1=0.1, omb2=0.001, eps=1e-8, wd=0.01, grad_scale=1.0, max_norm=1.0,
             clip=1, skip=0, zero=1, ws=A, ws_bytes=None, stream=None)
    a.update(over)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = _lib.lib().fastmax_hip_adamw_workspace(max(n, 1))
    return _lib.lib().fastmax_hip_adamw_update(*a.values())


def _norm(g=A, g_dtype=_lib.F32, n=5000, ws=A, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = _lib.lib().fastmax_hip_adamw_workspace(max(n, 1))
    return _lib.lib().fastmax_hip_adamw_norm(g, g_dtype, n, 1.0, ws, ws_bytes, None)


def test_update_rejects_bad_calls_before_any_launch():
    for missing in ("g", "m", "v", "master", "segments", "chunks", "ws"):
        assert _update(**{missing: None}) == _lib.E_NULL, missing
    for dt in (-1, 3):
        assert _update(g_dtype=dt) == _lib.E_BAD_DTYPE
    for n in (0, -4):
        assert _update(n=n) == _lib.E_BAD_SHAPE
    chunk = optim.chunk_elems()
    for n_chunks in (0, -1, 2 ** 31, 5000 // chunk, 5001):        # none, too many for the grid, too few to cover n, more than n
        assert _update(n_chunks=n_chunks) == _lib.E_BAD_SHAPE, n_chunks
    assert _update(n=3 * 2 ** 31, n_chunks=2 ** 31) == _lib.E_BAD_SHAPE
    for n_segments in (0, 5001):
        assert _update(n_segments=n_segments) == _lib.E_BAD_SHAPE
    for misaligned in ("m", "v", "master", "ws"):
        assert _update(**{misaligned: A + 4}) == _lib.E_ALIGNMENT, misaligned
    assert _update(g=A + 2) == _lib.E_ALIGNMENT and _update(g=A + 1, g_dtype=_lib.BF16) == _lib.E_ALIGNMENT
    assert _update(lr_ptr=A + 2) == _lib.E_ALIGNMENT
    need = _lib.lib().fastmax_hip_adamw_workspace(5000)
    assert _update(ws_bytes=need - 1) == _lib.E_WORKSPACE and _update(ws_bytes=0) == _lib.E_WORKSPACE


def test_norm_rejects_bad_calls_before_any_launch():
    assert _norm(g=None) == _lib.E_NULL and _norm(ws=None) == _lib.E_NULL
    assert _norm(g_dtype=3) == _lib.E_BAD_DTYPE and _norm(g_dtype=-1) == _lib.E_BAD_DTYPE
    assert _norm(n=0) == _lib.E_BAD_SHAPE and _norm(n=-1) == _lib.E_BAD_SHAPE
    assert _norm(ws=A + 8) == _lib.E_ALIGNMENT and _norm(g=A + 1) == _lib.E_ALIGNMENT
    assert _norm(ws_bytes=_lib.lib().fastmax_hip_adamw_workspace(5000) - 1) == _lib.E_WORKSPACE


# ---- 3. the chunk table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [SIZES, "3chunk+5"], ids=["six_segments", "one_long_segment"])
def test_chunk_table_covers_every_index_once_and_respects_segments(sizes):
    chunk = optim.chunk_elems()
    if sizes == "3chunk+5":
        sizes = [3 * chunk + 5]
    table = optim.chunk_table(sizes, chunk)
    assert table.dtype.itemsize == 16 and optim.SEGMENT_RECORD.itemsize == 32
    n = sum(sizes)
    hits = np.zeros(n, dtype=np.int64)
    bounds = np.cumsum([0] + sizes)
    for c in table:
        start, seg, ln = int(c["start"]), int(c["segment"]), int(c["len"])
        assert 1 <= ln <= chunk
        assert bounds[seg] <= start and start + ln <= bounds[seg + 1], "a chunk crosses its segment's boundary"
        hits[start:start + ln] += 1
    assert (hits == 1).all()
    assert len(table) == sum(-(-s // chunk) for s in sizes)
    segs = optim.segment_table([A] * len(sizes), sizes, [_lib.F32] * len(sizes))
    assert list(segs["offset"]) == list(bounds[:-1]) and list(segs["numel"]) == sizes


def test_chunk_table_refuses_empty_segments():
    with pytest.raises(ValueError):
        optim.chunk_table([4, 0, 3], 1024)
    with pytest.raises(ValueError):
        optim.chunk_table([4], 0)


# ---- 4. the host contract ------------------------------------------------------------------------------------------------------
def _params(dtypes, seed=0, sizes=SIZES):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(((torch.rand(s, generator=g) - 0.5) * 0.8).to(dt)) for s, dt in zip(sizes, dtypes)]


MIXED = [torch.float32, torch.bfloat16, torch.float16, torch.float32, torch.bfloat16, torch.float32]


def _grads(n, steps, seed=1):
    g = torch.Generator().manual_seed(seed)
    out = torch.randn(steps, n, generator=g) * 0.1
    out[:, ::97] = 0.0                           # a few exactly-zero gradients
    return out


def test_value_errors():
    t = torch.nn.Parameter(torch.randn(6, 4).t())                    # a transposed view: not contiguous
    with pytest.raises(ValueError, match="contiguous"):
        optim.FlatAdamW(dp.FlatGradBucket([t]))
    opt = optim.FlatAdamW(dp.FlatGradBucket(_params(MIXED)))
    with pytest.raises(ValueError, match="one param group"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(3))]})
    assert len(opt.param_groups) == 1 and opt.param_groups[0]["params"] == opt.bucket.params
    with pytest.raises(ValueError, match="lr should be"):
        opt.step(lr=torch.tensor(1e-3, dtype=torch.float64))
    with pytest.raises(ValueError, match="lr should be"):
        opt.step(lr=1e-3)
    with pytest.raises(ValueError):
        optim.FlatAdamW(dp.FlatGradBucket(_params(MIXED)), betas=(0.9, 1.0))
    with pytest.raises(ValueError):
        optim.FlatAdamW(dp.FlatGradBucket([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))]))


def test_lambda_lr_drives_the_one_group():
    opt = optim.FlatAdamW(dp.FlatGradBucket(_params(MIXED)), lr=1e-2)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda step: (step + 1) / 4)
    seen = []
    for _ in range(3):
        seen.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    assert seen == pytest.approx([0.0025, 0.005, 0.0075]) and opt.step_count() == 3


def _run(opt, grads, **kw):
    for g in grads:
        opt.bucket.flat.copy_(g)
        opt.step(**kw)


def _bits(opt):
    out = [opt.m.clone(), opt.v.clone()] + [p.detach().clone() for p in opt.bucket.params]
    return out + ([] if opt.master is None else [opt.master.clone()])


def test_state_dict_round_trip_continues_bit_for_bit():
    grads = _grads(sum(SIZES), 4)
    a = optim.FlatAdamW(dp.FlatGradBucket(_params(MIXED)), lr=1e-2)
    _run(a, grads[:2], max_norm=0.5)
    state = a.state_dict()
    weights = [p.detach().clone() for p in a.bucket.params]
    assert state["step"] == 2 and state["skipped"] == 0 and set(state) == {"m", "v", "master", "step", "skipped", "param_groups"}
    _run(a, grads[2:], max_norm=0.5)
    b = optim.FlatAdamW(dp.FlatGradBucket([torch.nn.Parameter(w.clone()) for w in weights]), lr=5.0)
    b.load_state_dict(state)
    assert b.step_count() == 2 and b.param_groups[0]["lr"] == 1e-2
    _run(b, grads[2:], max_norm=0.5)
    assert a.step_count() == b.step_count() == 4
    for x, y in zip(_bits(a), _bits(b)):
        assert torch.equal(x, y)
    other = optim.FlatAdamW(dp.FlatGradBucket(_params(MIXED[:3], sizes=SIZES[:3])))
    with pytest.raises(ValueError, match="another bucket"):
        other.load_state_dict(state)


def test_refresh_master_rereads_the_16_bit_parameters():
    opt = optim.FlatAdamW(dp.FlatGradBucket(_params(MIXED)))
    p = opt.bucket.params[1]                                           # bf16, flat offset 1
    assert torch.equal(opt.master[1:8], p.detach().float())
    with torch.no_grad():
        p.fill_(0.25)
    opt.refresh_master()
    assert torch.equal(opt.master[1:8], torch.full((7,), 0.25)) and float(opt.master[0]) == 0.0    # fp32 parameters: no master


# ---- 5. the CPU rehearsal against the float64 restatement -------------------------------------------------------------------------
@pytest.mark.parametrize("bucket_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("wd,grad_scale,max_norm", [(0.0, 1.0, None), (0.01, 0.5, 1.0), (0.01, 1.0, 1e4)])
def test_rehearsal_matches_the_restatement(bucket_dtype, wd, grad_scale, max_norm):
    params = _params(MIXED)
    bucket = dp.FlatGradBucket(params, dtype=bucket_dtype)
    opt = optim.FlatAdamW(bucket, lr=1e-2, weight_decay=wd)
    ref = AdamWRef(torch.cat([p.detach().float().reshape(-1) for p in params]).numpy(), lr=1e-2, weight_decay=wd)
    for g in _grads(sum(SIZES), 6):
        bucket.flat.copy_(g)
        fed = bucket.flat.double().numpy().copy()                      # the bucket's own rounded values
        opt.step(grad_scale=grad_scale, max_norm=max_norm)
        ref.step(fed, grad_scale=grad_scale, max_norm=max_norm)
        assert float(bucket.flat.abs().sum()) == 0.0
    if max_norm is not None:
        assert (ref.coef < 1.0) == (max_norm == 1.0)                   # 1.0 clips these gradients, 1e4 does not
        assert opt.last_norm() == pytest.approx(ref.norm, rel=1e-5)
    assert opt.step_count() == 6 and np.abs(ref.p).max() <= 0.5
    off = 0
    for p in params:
        want = ref.p[off:off + p.numel()]
        got = p.detach() if p.dtype == torch.float32 else opt.master[off:off + p.numel()]
        assert float(np.abs(got.double().numpy() - want).max()) <= PARITY_TOL
        if p.dtype != torch.float32:
            assert torch.equal(p.detach(), opt.master[off:off + p.numel()].to(p.dtype))
        off += p.numel()


def test_rehearsal_skips_a_non_finite_step():
    opt = optim.FlatAdamW(dp.FlatGradBucket(_params(MIXED)), lr=1e-2, skip_nonfinite=True)
    grads = _grads(sum(SIZES), 2)
    _run(opt, grads[:1])
    before = _bits(opt)
    bad = grads[1].clone()
    bad[1030] = float("inf")
    _run(opt, [bad])
    assert opt.skipped() == 1 and opt.step_count() == 1 and float(opt.bucket.flat.abs().sum()) == 0.0
    for x, y in zip(before, _bits(opt)):
        assert torch.equal(x, y)
