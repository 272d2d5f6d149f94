"""Second-order decode state cache (decode.py FastmaxDecodeState(p=2), csrc/fastmax_decode_p2.hip) on an MI355X: prefill plus
single-token steps against masked p=2 fastmax over the extended sequence (C oracle, float64 blockwise rows), grouped-query
heads, strided inputs and run-to-run bitwise reproducibility.

Tolerances are those of the first-order decode test (test_fastmax_gpu.py): fp32 2e-4, bf16 8e-3, f16 2e-3, each step row
against that row's own magnitude."""
import numpy as np
import pytest
import torch

import blockwise as bw
from conftest import rel_err
from oracle import c_oracle, fastmax_oracle as orc

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-4, torch.bfloat16: 8e-3, torch.float16: 2e-3}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from fastmax_experiments_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _state(*a, **kw):
    from fastmax_experiments_amd.decode import FastmaxDecodeState
    return FastmaxDecodeState(*a, p=2, **kw)


def _row_err(got, ref):
    """worst over the rows (last axis = D) of max|got - ref| / max|ref| of that row"""
    got = np.asarray(got, np.float64).reshape(-1, ref.shape[-1])
    ref = np.asarray(ref, np.float64).reshape(-1, ref.shape[-1])
    return float((np.abs(got - ref).max(1) / np.maximum(np.abs(ref).max(1), 1e-6)).max())


def _run(st, q, k, v, T):
    """prefill over the first T tokens, then one step per remaining token -> (prefill o, stacked step outputs (B,H,S,D))"""
    o = st.prefill(q[:, :, :T], k[:, :, :T], v[:, :, :T])
    steps = [st.step(q[:, :, t:t + 1], k[:, :, t:t + 1], v[:, :, t:t + 1]) for t in range(T, q.shape[2])]
    return o, torch.cat(steps, dim=2)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,H,T,D", [(2, 3, 200, 64), (1, 2, 70, 32), (1, 2, 130, 128), (1, 2, 77, 40)])
def test_prefill_and_steps_match_masked_forward(B, H, T, D, dt):
    g = torch.Generator().manual_seed(T + D)
    q, k, v = (torch.randn(B, H, T + 6, D, generator=g).to(dt) for _ in range(3))
    ref, _ = c_oracle.fwd(q.float().numpy(), k.float().numpy(), v.float().numpy(), mask=True, p=2)
    st = _state(B, H, D, "cuda")
    o, steps = _run(st, q.cuda(), k.cuda(), v.cuda(), T)
    assert o.shape == (B, H, T, D) and steps.shape == (B, H, 6, D) and steps.dtype == dt
    assert rel_err(o.float().cpu().numpy(), ref[:, :, :T]) < TOL[dt]
    err = _row_err(steps.float().cpu().numpy(), ref[:, :, T:])
    print(f"p2 decode ({B},{H},{T},{D}) {dt}: worst step row {err:.3e}")
    assert err < TOL[dt]
    assert st.count == T + 6


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_head_size_without_whole_16_byte_rows(dt):
    """D = 33: rows that are not whole 16-byte pieces take the prefill kernel's element loads"""
    B, H, T, D = 1, 2, 95, 33
    g = torch.Generator().manual_seed(33)
    q, k, v = (torch.randn(B, H, T + 3, D, generator=g).to(dt) for _ in range(3))
    ref, _ = c_oracle.fwd(q.float().numpy(), k.float().numpy(), v.float().numpy(), mask=True, p=2)
    _, steps = _run(_state(B, H, D, "cuda"), q.cuda(), k.cuda(), v.cuda(), T)
    assert _row_err(steps.float().cpu().numpy(), ref[:, :, T:]) < TOL[dt]


@pytest.mark.parametrize("Hkv", [2, 1])
def test_grouped_query_heads(Hkv):
    B, H, T, D, S = 2, 8, 150, 64, 5
    g = torch.Generator().manual_seed(Hkv)
    q = torch.randn(B, H, T + S, D, generator=g)
    k, v = (torch.randn(B, Hkv, T + S, D, generator=g) for _ in range(2))
    ke, ve = (t.repeat_interleave(H // Hkv, dim=1) for t in (k, v))
    ref, _ = c_oracle.fwd(q.numpy(), ke.numpy(), ve.numpy(), mask=True, p=2)
    st = _state(B, H, D, "cuda", n_query_groups=Hkv)
    o, steps = _run(st, q.cuda(), k.cuda(), v.cuda(), T)
    assert rel_err(o.cpu().numpy(), ref[:, :, :T]) < TOL[torch.float32]
    assert _row_err(steps.cpu().numpy(), ref[:, :, T:]) < TOL[torch.float32]
    # the same sequence through a cache with one record per query head over the expanded K, V
    full = _state(B, H, D, "cuda")
    o_f, steps_f = _run(full, q.cuda(), ke.cuda(), ve.cuda(), T)
    assert full.state.numel() > st.state.numel()
    assert _row_err(steps.cpu().numpy(), steps_f.cpu().numpy()) < 1e-5
    assert _row_err(o.cpu().numpy(), o_f.cpu().numpy()) < 1e-5


@pytest.mark.parametrize("D", [64, 128])
def test_steps_after_long_prefill_blockwise(D):
    B, H, T, S = 1, 2, 4096, 64
    g = torch.Generator().manual_seed(T + D)
    q, k, v = (torch.randn(B, H, T + S, D, generator=g).to(torch.bfloat16) for _ in range(3))
    nt = orc.effective_normalize_term(D)
    st = _state(B, H, D, "cuda")
    _, steps = _run(st, q.cuda(), k.cuda(), v.cuda(), T)
    for h in range(H):
        ro, _ = bw.dense_rows(*(t[0, h].double().numpy() for t in (q, k, v)), nt=nt, p=2, mask=True)
        err, r0, _, scale = bw.worst_block(steps[0, h].double().cpu().numpy(), ro[T:], block=1)
        print(f"p2 decode after {T} tokens, D={D}, head {h}: worst step row {err:.3e} (step {r0}, max|ref| {scale:.3e})")
        assert err <= TOL[torch.bfloat16], (h, r0, err)


def test_strided_inputs_bit_identical_to_contiguous():
    B, H, Hkv, T, S, D = 2, 4, 2, 90, 4, 64
    g = torch.Generator().manual_seed(7)
    packed = torch.randn(B, T + S, H + 2 * Hkv, D, generator=g).to(torch.bfloat16).cuda()      # (B, N, heads, D) storage
    q, k, v = (packed[:, :, a:b].transpose(1, 2) for a, b in ((0, H), (H, H + Hkv), (H + Hkv, H + 2 * Hkv)))
    assert not (q.is_contiguous() or k.is_contiguous() or v.is_contiguous())
    s1, s2 = _state(B, H, D, "cuda", n_query_groups=Hkv), _state(B, H, D, "cuda", n_query_groups=Hkv)
    o1, st1 = _run(s1, q, k, v, T)
    o2, st2 = _run(s2, q.contiguous(), k.contiguous(), v.contiguous(), T)
    assert torch.equal(st1, st2) and torch.equal(o1, o2)
    assert torch.equal(s1.state, s2.state)


def test_bitwise_reproducible():
    B, H, Hkv, T, S, D = 1, 8, 2, 300, 5, 128
    g = torch.Generator().manual_seed(11)
    q = torch.randn(B, H, T + S, D, generator=g).to(torch.bfloat16).cuda()
    k, v = (torch.randn(B, Hkv, T + S, D, generator=g).to(torch.bfloat16).cuda() for _ in range(2))
    runs = []
    for _ in range(2):
        st = _state(B, H, D, "cuda", n_query_groups=Hkv)
        o, steps = _run(st, q, k, v, T)
        torch.cuda.synchronize()
        runs.append((o, steps, st.state.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
