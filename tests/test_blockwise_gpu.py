"""Long-sequence parity, block by block: the causal scans carry a D x D prefix state across 64-row chunks and sequence-split
segments, and a fault there shows in the late rows, whose magnitude falls like 1/sqrt(i).  Each case runs forward and
backward through the public ``fastmax`` / ``fastmax_hack`` and checks every 64-row block against the float64 references of
tests/blockwise.py relative to that block's own magnitude (tests/test_blockwise_cpu.py shows the faults this catches and
the per-tensor metric does not).

Tolerances (per block; forward / backward).  The result's own rounding is 2^-8 = 3.9e-3 of an element in bf16 and
2^-11 = 4.9e-4 in fp16, never more than that of its block's max; the kernels add the bf16 operands of their matrix products
(q, k, P = 1 + a s and the single-part state image, fastmax_mfma_bf16.hip:27-31: 2^-9 relative each, averaged over D-term
sums) or split-bf16 operands (~2^-16 per product) in fp32 accumulation for fp32.  Measured worst blocks sit at the result's
rounding (bf16 3.6e-3 .. 5.8e-3, fp16 4.4e-4 .. 4.8e-4, fp32 <= 2.4e-5), so:
  bf16  8e-3 / 1e-2    -- 2x / 2.5x the result's rounding.
  fp16  2e-3 / 2e-3    -- 4x the result's rounding.
  fp32  2e-4 / 2e-4    -- TOL_FWD of test_fastmax_gpu.py for both: ~8x the measured error.
  linearmax bf16 gradients keep 2.5e-2: the one-row fix-up that adds the prologue's dL/dM term to the row n* attaining the
  max-norm (fastmax_normalize.hip, normalize_bwd_fixadd_kernel) makes that row ~50x larger than its neighbours and carries
  the error of the sum T = sum dS . s (fastmax_mfma_bwd_lin.hip, kpart_dot) over the whole head: 2.1e-2 measured at config 5.
None of them is looser than the per-tensor number the same family is held to elsewhere in the suite.
"""
import numpy as np
import pytest
import torch

import blockwise as bw
from oracle import fastmax_oracle as orc

pytestmark = pytest.mark.gpu

TOL = {torch.bfloat16: (8e-3, 1e-2), torch.float16: (2e-3, 2e-3), torch.float32: (2e-4, 2e-4)}
TOL_LINEARMAX_BWD = 2.5e-2


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from fastmax_experiments_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _np(t):
    return t.detach().double().cpu().numpy()


def _check(case, name, got, ref, tol, **kw):
    err, r0, r1, scale = bw.worst_block(got, ref, **kw)
    print(f"BLOCKWISE {case} {name} worst {err:.3e} rows {r0}:{r1} tol {tol:.1e}")
    assert err <= tol, f"{case} {name}: rows {r0}:{r1} err {err:.3e} > {tol:.1e} (block max|ref| {scale:.3e})"


def _inputs(shape, dt, seed, nk=None):
    g = torch.Generator().manual_seed(seed)
    B, H, N, D = shape
    q, go = (torch.randn(B, H, N, D, generator=g).to(dt) for _ in range(2))
    k, v = (torch.randn(B, H, N if nk is None else nk, D, generator=g).to(dt) for _ in range(2))
    return q, k, v, go


def _split_ran(q, k, v, nt):
    """the p = 1 masked forward of this problem keeps sequence-split prefix states (split_plan, fastmax_mfma_split.hip)"""
    from fastmax_experiments_amd import ops
    return ops.forward(q, k, v, 1, True, nt, 0.0, q.dtype, keep_states=True)[2] is not None


def test_config5_linearmax_16k_blockwise():
    """BASELINE config 5: linearmax (1,32,16384,128) bf16, 8 segments of 2048 rows.  Inference route: prologue fused into
    fastmax_mfma_bf16.hip (mfma_bf16_supported); training route: _LinearmaxP1 (fastmax_hip_linearmax_train_supported:
    mfma_gen_supported + lin_bwd_supported -> fastmax_mfma_bwd_lin.hip).  Heads 0, 17, 31."""
    from attention_mechanisms.fastmax_hack import fastmax_hack
    B, H, N, D = 1, 32, 16384, 128
    g = torch.Generator(device="cuda").manual_seed(5)
    q, k, v, go = (torch.randn(B, H, N, D, device="cuda", generator=g).to(torch.bfloat16) for _ in range(4))
    assert _split_ran(q, k, v, 8 * D ** 0.5)
    with torch.no_grad():
        oi = fastmax_hack(q, k, v, p=1, mask=True)
    qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
    o = fastmax_hack(qq, kk, vv, p=1, mask=True)
    o.backward(go)
    tf, tb = TOL[torch.bfloat16][0], TOL_LINEARMAX_BWD
    for h in (0, 17, 31):
        qh, kh, vh, gh = (_np(t[0, h]) for t in (q, k, v, go))
        ro, _ = bw.linearmax_fwd(qh, kh, vh)
        _check("config5", f"o_inference h{h}", _np(oi[0, h]), ro, tf)
        _check("config5", f"o_training h{h}", _np(o[0, h]), ro, tf)
        for t, r, n in zip((qq, kk, vv), bw.linearmax_bwd(qh, kh, vh, gh), ("dq", "dk", "dv")):
            _check("config5", f"{n} h{h}", _np(t.grad[0, h]), r, tb)


# p = 1 masked through fastmax(); families from the *_supported predicates (fwd -> bwd):
#   bf16, D <= 128             mfma_bf16_supported  -> fastmax_mfma_bf16.hip    | lin_bwd_supported -> fastmax_mfma_bwd_lin.hip
#   fp16, D <= 64              mfma_gen_supported   -> fastmax_mfma_gen.hip     | lin_bwd_supported -> fastmax_mfma_bwd_lin.hip
#   fp32, D == 64              mfma_p1_supported    -> fastmax_mfma_v2.hip      | lin_bwd_supported -> fastmax_mfma_bwd_lin.hip
#                              (a head whose byte span reaches 2 GiB -> fastmax_mfma_gen.hip, test_p1_f32_head_span_2gib_blockwise)
#   fp32 / fp16, 64 < D <= 128 mfma_d128_2p_supported -> fastmax_mfma_d128_2p.hip | scan_bwd_supported -> fastmax_scan_d128_2p.hip
# split: split_plan (fastmax_mfma_split.hip) cuts the sequence when B*H is far below the target; (16,32,4096,64) is not cut
P1_CASES = [
    # shape, dtype, heads checked (None: all), split expected
    ((1, 2, 16384, 64), torch.bfloat16, None, True),     # 32 segments of 512 rows
    ((1, 2, 16384, 64), torch.float16, None, True),
    ((1, 4, 4096, 64), torch.float32, None, True),       # headline kernel, 16 segments of 256 rows
    ((16, 32, 4096, 64), torch.float32, (0, 511), False),   # headline kernel, one segment per head
    ((1, 2, 8192, 128), torch.float32, None, True),      # two-part D = 128 forward and scan_bwd
    ((1, 2, 8192, 128), torch.float16, None, True),
    ((1, 3, 5000, 64), torch.bfloat16, None, True),      # ragged: 8-row last chunk, 4-chunk last segment
    ((1, 3, 5000, 64), torch.float32, None, True),
    ((1, 2, 6001, 128), torch.bfloat16, None, True),     # ragged: 49-row last chunk
    ((1, 2, 6001, 128), torch.float32, None, True),
]


@pytest.mark.parametrize("shape,dt,heads,split", P1_CASES, ids=lambda x: str(x).replace(" ", ""))
def test_p1_masked_scans_blockwise(shape, dt, heads, split):
    from attention_mechanisms.fastmax import fastmax
    B, H, N, D = shape
    q, k, v, go = _inputs(shape, dt, N + D)
    nt = orc.effective_normalize_term(D)
    qq, kk, vv = (t.cuda().requires_grad_(True) for t in (q, k, v))
    assert _split_ran(qq.detach(), kk.detach(), vv.detach(), nt) == split
    o = fastmax(qq, kk, vv, mask=True, p=1)
    o.backward(go.cuda())
    tf, tb = TOL[dt]
    case = f"p1_{B}x{H}x{N}x{D}_{str(dt)[6:]}"
    for bh in (range(B * H) if heads is None else heads):
        b, h = divmod(bh, H)
        qh, kh, vh, gh = (_np(t[b, h]) for t in (q, k, v, go))
        ro, _ = bw.p1_causal_fwd(qh, kh, vh, nt)
        _check(case, f"o h{bh}", _np(o[b, h]), ro, tf)
        for t, r, n in zip((qq, kk, vv), bw.p1_causal_bwd(qh, kh, vh, gh, nt), ("dq", "dk", "dv")):
            _check(case, f"{n} h{bh}", _np(t.grad[b, h]), r, tb)


def test_p1_f32_head_span_2gib_blockwise():
    """fp32, D = 64 heads whose byte span reaches 2 GiB do not fit the 31-bit buffer offsets of the headline kernel
    (launch_fwd_mfma_p1, fastmax_mfma_v2.hip) and take the generic kernel (fastmax_mfma_gen.hip, 64-bit addresses), here
    with the sequence split of a lone head.  q, k, v are column views of (N, W) buffers, which ops._prep passes through."""
    from attention_mechanisms.fastmax import fastmax
    from fastmax_experiments_amd import ops
    N, W, D = 4096, 131072, 64
    q, k, v, _ = _inputs((1, 1, N, D), torch.float32, N + D + 1)
    nt = orc.effective_normalize_term(D)
    views = []
    for t in (q, k, v):
        buf = torch.zeros(N, W, device="cuda")
        buf[:, :D] = t[0, 0].cuda()
        views.append(buf[:, :D][None, None])
    for t in views:
        assert ops._prep(t, t.device) is t                               # no copy: the kernel sees the W-float row stride
        assert (N * t.stride(2)) * t.element_size() >= 2 ** 31           # past the 31-bit offsets of the headline kernel
    qv, kv, vv = views
    assert _split_ran(qv, kv, vv, nt)
    with torch.no_grad():
        o = fastmax(qv, kv, vv, mask=True, p=1)
    ro, _ = bw.p1_causal_fwd(_np(q[0, 0]), _np(k[0, 0]), _np(v[0, 0]), nt)
    _check(f"p1_span2GiB_1x1x{N}x{D}_float32", "o h0", _np(o[0, 0]), ro, TOL[torch.float32][0])


# p = 2 masked: quad32_supported -> fastmax_quad32_mfma.hip, quad32_bwd_supported -> fastmax_quad32_bwd.hip (32-wide tiles);
# unmasked p = 1: unmasked_lin_supported / unmasked_lin_bwd_supported -> the linear-form kernels of fastmax_mfma_split.hip.
# Blocks run along the queries for o, dq and along the keys for dk, dv.
DENSE_CASES = [
    # shape (B, H, Nq, D), Nk, p, mask, dtype
    ((1, 2, 4096, 128), 4096, 2, True, torch.bfloat16),
    ((1, 2, 4096, 64), 4096, 2, True, torch.float32),
    ((1, 2, 2048, 64), 8192, 1, False, torch.bfloat16),
    ((1, 2, 2048, 64), 8192, 1, False, torch.float32),
]


@pytest.mark.parametrize("shape,nk,p,mask,dt", DENSE_CASES, ids=lambda x: str(x).replace(" ", ""))
def test_tile_and_unmasked_kernels_blockwise(shape, nk, p, mask, dt):
    from attention_mechanisms.fastmax import fastmax
    B, H, N, D = shape
    q, k, v, go = _inputs(shape, dt, N + nk + D + p, nk)
    qq, kk, vv = (t.cuda().requires_grad_(True) for t in (q, k, v))
    o = fastmax(qq, kk, vv, mask=mask, p=p)
    o.backward(go.cuda().to(o.dtype))
    tf, tb = TOL[dt]
    case = f"p{p}_{'masked' if mask else 'unmasked'}_{N}x{nk}x{D}_{str(dt)[6:]}"
    for h in range(H):
        ro, _, *grads = bw.dense_rows(*(_np(t[0, h]) for t in (q, k, v, go)), p=p, mask=mask)
        _check(case, f"o h{h}", _np(o[0, h]), ro, tf)
        for t, r, n in zip((qq, kk, vv), grads, ("dq", "dk", "dv")):
            _check(case, f"{n} h{h}", _np(t.grad[0, h]), r, tb)


@pytest.mark.parametrize("D", [64, 128])
def test_decode_after_long_prefill_blockwise(D):
    """FastmaxDecodeState (decode.py): masked prefill of 4096 tokens (fastmax_mfma_bf16.hip + fastmax_hip_p1_prefill_state),
    then 64 single-token steps (fastmax_hip_p1_decode_step); each step's row against that row's own magnitude"""
    from fastmax_experiments_amd.decode import FastmaxDecodeState
    B, H, T, S = 1, 2, 4096, 64
    q, k, v, _ = _inputs((B, H, T + S, D), torch.bfloat16, T + D)
    nt = orc.effective_normalize_term(D)
    ref = np.stack([bw.p1_causal_fwd(*(_np(t[0, h]) for t in (q, k, v)), nt)[0] for h in range(H)])
    tf, _ = TOL[torch.bfloat16]
    st = FastmaxDecodeState(B, H, D, "cuda")
    qc, kc, vc = q.cuda(), k.cuda(), v.cuda()
    o = st.prefill(qc[:, :, :T], kc[:, :, :T], vc[:, :, :T])
    for h in range(H):
        _check(f"decode_d{D}", f"prefill h{h}", _np(o[0, h]), ref[h, :T], tf)
    steps = np.stack([_np(st.step(qc[:, :, t:t + 1], kc[:, :, t:t + 1], vc[:, :, t:t + 1])[0, :, 0]) for t in range(T, T + S)])
    _check(f"decode_d{D}", "steps", steps.reshape(S * H, D), ref[:, T:].transpose(1, 0, 2).reshape(S * H, D), tf, block=1)
