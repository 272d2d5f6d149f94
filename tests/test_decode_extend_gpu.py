"""Multi-token continuation of the second-order decode state cache (FastmaxDecodeState.extend, prefill(chunk=...),
csrc/fastmax_decode_p2.hip) on an MI355X.  The reference is masked p=2 fastmax over the WHOLE sequence (C oracle on the
fp32-upcast inputs, float64 blockwise rows for the long runs); steps taken after the extends prove the accumulated state.

Error measure and tolerances are those of test_decode_p2_gpu.py: the worst row against that row's own magnitude,
fp32 2e-4, bf16 8e-3, f16 2e-3."""
import ctypes

import numpy as np
import pytest
import torch

import blockwise as bw
from oracle import c_oracle, fastmax_oracle as orc

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-4, torch.bfloat16: 8e-3, torch.float16: 2e-3}
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


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


def _np(t):
    return t.float().cpu().numpy()


def _oracle(q, k, v):
    ref, _ = c_oracle.fwd(_np(q), _np(k), _np(v), mask=True, p=2)
    return ref


def _feed(st, q, k, v, plan):
    """plan: list of ("prefill" | "extend" | "step", n tokens) -> outputs of every piece, concatenated along the sequence"""
    out, pos = [], 0
    for what, n in plan:
        if what == "step":
            for t in range(pos, pos + n):
                out.append(st.step(q[:, :, t:t + 1], k[:, :, t:t + 1], v[:, :, t:t + 1]))
        else:
            out.append(getattr(st, what)(q[:, :, pos:pos + n], k[:, :, pos:pos + n], v[:, :, pos:pos + n]))
        pos += n
    assert st.count == pos
    return torch.cat(out, dim=2)


EXT = [("extend", 1), ("extend", 7), ("extend", 64), ("extend", 200), ("step", 4)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,H,T,D", [(2, 3, 200, 64), (1, 2, 70, 32), (1, 2, 130, 128), (1, 2, 77, 40), (1, 2, 95, 33)])
def test_prefill_extends_then_steps_match_masked_forward(B, H, T, D, dt):
    N = T + 276
    g = torch.Generator().manual_seed(T + D)
    q, k, v = (torch.randn(B, H, N, D, generator=g).to(dt) for _ in range(3))
    ref = _oracle(q, k, v)
    st = _state(B, H, D, "cuda")
    o = _feed(st, q.cuda(), k.cuda(), v.cuda(), [("prefill", T)] + EXT)
    assert o.shape == (B, H, N, D) and o.dtype == dt
    got, pos = _np(o), T
    for what, n in EXT:
        err = _row_err(got[:, :, pos:pos + n], ref[:, :, pos:pos + n])
        print(f"p2 extend ({B},{H},{T},{D}) {dt}: {what} {n} tokens after {pos}: worst row {err:.3e}")
        assert err < TOL[dt], (what, n, pos, err)
        pos += n
    assert _row_err(got[:, :, :T], ref[:, :, :T]) < TOL[dt]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,H,T,D", [(2, 3, 150, 64), (1, 2, 9, 128), (1, 4, 300, 40), (1, 2, 50, 33)])
def test_extend_into_fresh_state_is_the_masked_forward(B, H, T, D, dt):
    g = torch.Generator().manual_seed(T * D)
    q, k, v = (torch.randn(B, H, T + 3, D, generator=g).to(dt) for _ in range(3))
    ref = _oracle(q, k, v)
    st = _state(B, H, D, "cuda")
    o = _feed(st, q.cuda(), k.cuda(), v.cuda(), [("extend", T), ("step", 3)])
    err = _row_err(_np(o), ref)
    print(f"p2 extend into an empty state ({B},{H},{T},{D}) {dt}: worst row {err:.3e}")
    assert err < TOL[dt]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", [64, 128])
def test_extend_by_one_token_and_step_agree(D, dt):
    B, H, T = 2, 3, 120
    g = torch.Generator().manual_seed(D)
    q, k, v = (torch.randn(B, H, T + 5, D, generator=g).to(dt) for _ in range(3))
    ref = _oracle(q, k, v)
    qc, kc, vc = q.cuda(), k.cuda(), v.cuda()
    a = _feed(_state(B, H, D, "cuda"), qc, kc, vc, [("prefill", T), ("extend", 1), ("step", 4)])
    b = _feed(_state(B, H, D, "cuda"), qc, kc, vc, [("prefill", T), ("step", 1), ("step", 4)])
    for name, o in (("extend", a), ("step", b)):
        e1 = _row_err(_np(o)[:, :, T:T + 1], ref[:, :, T:T + 1])
        e4 = _row_err(_np(o)[:, :, T + 1:], ref[:, :, T + 1:])
        print(f"p2 D={D} {dt}: token {T} by {name}: {e1:.3e}, the 4 steps after it: {e4:.3e}")
        assert e1 < TOL[dt] and e4 < TOL[dt], (name, e1, e4)


@pytest.mark.parametrize("Hkv", [2, 1])
def test_grouped_query_heads(Hkv):
    B, H, T, D = 2, 8, 150, 64
    plan = [("prefill", T), ("extend", 5), ("extend", 40), ("extend", 1), ("step", 4)]
    N = sum(n for _, n in plan)
    g = torch.Generator().manual_seed(Hkv)
    q = torch.randn(B, H, N, D, generator=g)
    k, v = (torch.randn(B, Hkv, N, D, generator=g) for _ in range(2))
    ke, ve = (t.repeat_interleave(H // Hkv, dim=1) for t in (k, v))
    ref = _oracle(q, ke, ve)
    st = _state(B, H, D, "cuda", n_query_groups=Hkv)
    o = _feed(st, q.cuda(), k.cuda(), v.cuda(), plan)
    err = _row_err(_np(o)[:, :, T:], ref[:, :, T:])
    print(f"p2 extend, {Hkv} KV heads under {H}: worst row {err:.3e}")
    assert err < TOL[torch.float32]
    # the same sequence through a cache with one record per query head over the repeated K, V
    full = _state(B, H, D, "cuda")
    o_f = _feed(full, q.cuda(), ke.cuda(), ve.cuda(), plan)
    assert full.state.numel() > st.state.numel()
    assert _row_err(_np(o), _np(o_f)) < 1e-5


def test_strided_inputs_bit_identical_to_contiguous():
    B, H, Hkv, D = 2, 4, 2, 64
    plan = [("prefill", 90), ("extend", 8), ("extend", 33), ("extend", 300), ("step", 3)]
    N = sum(n for _, n in plan)
    g = torch.Generator().manual_seed(7)
    packed = torch.randn(B, N, H + 2 * Hkv, D, generator=g).to(torch.bfloat16).cuda()      # (B, N, heads, D) storage
    q, k, v = (packed[:, :, a:b].transpose(1, 2) for a, b in ((0, H), (H, H + Hkv), (H + Hkv, H + 2 * Hkv)))
    assert not (q.is_contiguous() or k.is_contiguous() or v.is_contiguous())
    s1, s2 = _state(B, H, D, "cuda", n_query_groups=Hkv), _state(B, H, D, "cuda", n_query_groups=Hkv)
    o1 = _feed(s1, q, k, v, plan)
    o2 = _feed(s2, q.contiguous(), k.contiguous(), v.contiguous(), plan)
    assert torch.equal(o1, o2)
    assert torch.equal(s1.state, s2.state)
    ref = _oracle(q, k.repeat_interleave(H // Hkv, dim=1), v.repeat_interleave(H // Hkv, dim=1))
    assert _row_err(_np(o1)[:, :, 90:], ref[:, :, 90:]) < TOL[torch.bfloat16]


@pytest.mark.parametrize("B,H,Hkv,D,plan", [
    (1, 8, 2, 128, [("prefill", 300), ("extend", 8), ("extend", 130), ("step", 2)]),
    (1, 2, 2, 64, [("prefill", 64), ("extend", 8), ("step", 2)]),             # B = 1, T = 8: the reduction is split
    (2, 4, 4, 64, [("extend", 700), ("extend", 8)]),
])
def test_bitwise_reproducible(B, H, Hkv, D, plan):
    from fastmax_experiments_amd import _lib
    N = sum(n for _, n in plan)
    g = torch.Generator().manual_seed(11)
    q = torch.randn(B, H, N, D, generator=g).to(torch.bfloat16).cuda()
    k, v = (torch.randn(B, Hkv, N, D, generator=g).to(torch.bfloat16).cuda() for _ in range(2))
    runs = []
    for _ in range(2):
        st = _state(B, H, D, "cuda", n_query_groups=Hkv)
        o = _feed(st, q, k, v, plan)
        torch.cuda.synchronize()
        runs.append((o, st.state.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    ref = _oracle(q, k.repeat_interleave(H // Hkv, dim=1), v.repeat_interleave(H // Hkv, dim=1))
    assert _row_err(_np(runs[0][0]), ref) < TOL[torch.bfloat16]


@pytest.mark.parametrize("D", [64, 128])
def test_chunked_prefill_long_sequence_blockwise(D):
    B, H, N, S = 1, 2, 8192, 8
    g = torch.Generator().manual_seed(N + D)
    q, k, v = (torch.randn(B, H, N + S, D, generator=g).to(torch.bfloat16) for _ in range(3))
    nt = orc.effective_normalize_term(D)
    st = _state(B, H, D, "cuda")
    qc, kc, vc = q.cuda(), k.cuda(), v.cuda()
    o = st.prefill(qc[:, :, :N], kc[:, :, :N], vc[:, :, :N], chunk=1024)
    assert o.shape == (B, H, N, D) and st.count == N
    steps = torch.cat([st.step(qc[:, :, t:t + 1], kc[:, :, t:t + 1], vc[:, :, t:t + 1]) for t in range(N, N + S)], dim=2)
    for h in range(H):
        ro, _ = bw.dense_rows(*(t[0, h].double().numpy() for t in (q, k, v)), nt=nt, p=2, mask=True)
        err = bw.assert_blockwise(o[0, h].double().cpu().numpy(), ro[:N], TOL[torch.bfloat16],
                                  what=f"chunked p2 prefill D={D} head {h}")
        serr, r0, _, scale = bw.worst_block(steps[0, h].double().cpu().numpy(), ro[N:], block=1)
        print(f"chunked p2 prefill N={N} D={D} head {h}: worst 64-row block {err:.3e}; worst later step {serr:.3e} (step {r0})")
        assert serr <= TOL[torch.bfloat16], (h, r0, serr, scale)


@pytest.mark.parametrize("Hkv", [4, 2])
def test_unchunked_prefill_is_unchanged(Hkv):
    """chunk=None: the outputs are fastmax(mask=True, p=2) bit for bit and the state is what fastmax_hip_p2_prefill_state
    writes"""
    from fastmax_experiments_amd import _lib, ops
    from fastmax_experiments_amd.attention_mechanisms.fastmax import fastmax
    B, H, T, D = 2, 4, 333, 64
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B, H, T, D, generator=g).to(torch.bfloat16).cuda()
    k, v = (torch.randn(B, Hkv, T, D, generator=g).to(torch.bfloat16).cuda() for _ in range(2))
    st = _state(B, H, D, "cuda", n_query_groups=Hkv)
    st.state.fill_(3.0)                   # prefill overwrites the pair rows
    st_default = _state(B, H, D, "cuda", n_query_groups=Hkv)
    o = st.prefill(q, k, v, chunk=None)
    o_default = st_default.prefill(q, k, v)
    ke, ve = (t.repeat_interleave(H // Hkv, dim=1) for t in (k, v))
    assert torch.equal(o, fastmax(q, ke, ve, mask=True, p=2)) and torch.equal(o, o_default)
    L = _lib.lib()
    direct = torch.zeros_like(st.state)
    prob = ops._problem(k, k, k.dtype, k.dtype, 2, True, st.nt, 0.0)
    rc = L.fastmax_hip_p2_prefill_state(ctypes.byref(prob), k.data_ptr(), ops._strides(k), v.data_ptr(), ops._strides(v),
                                        direct.data_ptr(), ops._stream(k.device))
    assert rc == 0
    rows = L.fastmax_hip_p2_decode_state_bytes(B, Hkv, D) // 4
    P, DV = (D + 1) * (D + 2) // 2, (D + 4) // 4 * 4
    n = B * Hkv * P * DV
    assert n < rows
    assert torch.equal(st.state[:n], direct[:n]) and torch.equal(st_default.state[:n], direct[:n])
