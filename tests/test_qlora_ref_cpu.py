"""The element-wise bound of tests/qlora_ref.py, checked where no GPU is needed: for every case the GPU file runs, a CPU emulation
of a correct kernel (float32 products and sums of the bf16 operands, one rounding of the result) stays inside it, and the faults
a tile kernel can have -- a k term lost, the bias or the LoRA step lost, a ragged tile's row taking another row's operand, an
8-column chunk stored 8 columns off -- all break it.  The last test records why tests/test_lora_gpu.py alone is not enough."""
import math

import pytest
import torch

import qlora_ref as qr

BF16 = torch.bfloat16


def _rounded(c, dtype=BF16):
    """the operands as a bf16 kernel sees them"""
    return c.x.to(dtype), c.w.to(BF16), c.bias, c.ea, c.eb


LINEAR_SHAPES = ([(M, N, K, r) for (M, N, K) in qr.GEMM_SHAPES + [qr.GEMM_DQ_SHAPE] for r in qr.GEMM_RANKS]
                 + [(M, N, K, r) for (M, N, K, _) in qr.FWD_SHAPES for r in (0, 32)])


@pytest.mark.parametrize("M,N,K,rp", LINEAR_SHAPES)
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("out", [torch.bfloat16, torch.float32])
def test_emulated_linear_stays_inside_the_bound(M, N, K, rp, with_bias, out):
    c = qr.linear_case(M, N, K, rp)
    x, w, bias, ea, eb = _rounded(c)
    bias = bias if with_bias else None
    ref, S = qr.linear_ref(x, w, bias, ea, eb)
    got = qr.linear_emulate(x, w, bias, ea, eb, out)
    worst = qr.check_bound("emulation", got, ref, S, K + rp, qr.u_out(out))
    print(f"({M}, {N}, {K}) rank {rp} bias {with_bias} {out}: {worst}")
    # the three terms have one order of magnitude (the recipe): each alone is a visible share of y
    if N >= 64:                                                      # (too few columns for a standard deviation at N = 8)
        assert 0.5 < float((qr.f64(x) @ qr.f64(w).t()).std()) < 2.0 and 0.5 < float(c.bias.std()) < 2.0
        assert not rp or 0.5 < float((qr.f64(ea) @ qr.f64(eb).t()).std()) < 2.0


@pytest.mark.parametrize("M,N,K", qr.DX_SHAPES)
@pytest.mark.parametrize("out", [torch.bfloat16, torch.float32])
def test_emulated_input_gradient_stays_inside_the_bound(M, N, K, out):
    c = qr.linear_case(M, N, K, 0)
    dy, w = torch.randn(M, N, generator=torch.Generator().manual_seed(M + N)).to(BF16), c.w.to(BF16)
    ref, S = qr.linear_ref(dy, w.t())
    qr.check_bound("dx", qr.linear_emulate(dy, w.t().contiguous(), out_dtype=out), ref, S, N, qr.u_out(out))


@pytest.mark.parametrize("M", qr.DOWN_M)
@pytest.mark.parametrize("K", qr.DOWN_K)
@pytest.mark.parametrize("RP", qr.DOWN_RP)
def test_emulated_lora_down_stays_inside_the_bound(M, K, RP):
    c = qr.linear_case(M, RP, K, 0)
    x, bt = c.x.to(BF16), c.w.to(BF16)
    ref, S = qr.linear_ref(x, bt)
    qr.check_bound("down", qr.linear_emulate(x, bt), ref, S, K, qr.U_BF16)


@pytest.mark.parametrize("M,ncols,R,RP", qr.TN_SHAPES)
@pytest.mark.parametrize("out", [torch.bfloat16, torch.float32])
def test_emulated_lora_tn_stays_inside_the_bound(M, ncols, R, RP, out):
    g = torch.Generator().manual_seed(M + ncols + R)
    et = torch.randn(R, M, generator=g).to(BF16)
    x = torch.randn(M, ncols, generator=g).to(BF16)
    ref, S = qr.linear_ref(et, x.t())
    qr.check_bound("tn", qr.linear_emulate(et, x.t().contiguous(), out_dtype=out), ref, S, M, qr.u_out(out))


@pytest.mark.parametrize("R", qr.UP_R)
@pytest.mark.parametrize("N", qr.UP_N)
@pytest.mark.parametrize("M", qr.UP_M)
def test_emulated_lora_up_stays_inside_the_bound(R, N, M):
    g = torch.Generator().manual_seed(R + N + M)
    y0 = torch.randn(M, N, generator=g).to(BF16)
    e = torch.randn(M, R, generator=g).to(BF16)
    bn = (torch.randn(N, R, generator=g) / math.sqrt(R)).to(BF16)
    bias = torch.randn(N, generator=g)
    ref, S = qr.linear_ref(e, bn, bias)
    ref, S = ref + qr.f64(y0), S + qr.f64(y0).abs()
    got = ((y0.float() + bias) + e.float() @ bn.float().t()).to(BF16)
    qr.check_bound("up", got, ref, S, R + 2, qr.U_BF16)


@pytest.mark.parametrize("B,T,G,qpk,hs,rope_n,K", qr.ROPE_SHAPES)
@pytest.mark.parametrize("tables16", [False, True])
def test_emulated_rope_epilogue_stays_inside_its_bound(B, T, G, qpk, hs, rope_n, K, tables16):
    N = G * (qpk + 2) * hs
    c = qr.linear_case(B * T, N, K, 16)
    x, w, bias, ea, eb = _rounded(c)
    g = torch.Generator().manual_seed(T)
    ang = torch.rand(T, rope_n, generator=g) * 6.28
    cos, sin = ang.cos(), ang.sin()
    if tables16:
        cos, sin = cos.to(BF16).float(), sin.to(BF16).float()
    ref_y, S = qr.linear_ref(x, w, bias, ea, eb)
    by = qr.bound(ref_y, S, K + 16, qr.U_BF16)
    y = qr.linear_emulate(x, w, bias, ea, eb)
    got = qr.rope_apply(y.float(), cos, sin, T, G, qpk, hs, rope_n, tables16).to(BF16)
    ref = qr.rope_apply(ref_y, cos.double(), sin.double(), T, G, qpk, hs, rope_n)
    bnd = qr.rope_bound(ref_y, by, cos, sin, T, G, qpk, hs, rope_n, tables16)
    worst = qr.check_bound("rope", got, ref, None, 0, 0, tile=(256, hs), bnd=bnd)
    print(f"rope {(B, T, G, qpk, hs, rope_n, K)} tables16 {tables16}: {worst}")
    # a 256-row tile that takes its table row from row % 256 and not from row % T is caught
    wrong = qr.rope_apply(y.float(), cos.roll(1, 0), sin.roll(1, 0), T, G, qpk, hs, rope_n, tables16).to(BF16)
    with pytest.raises(AssertionError, match="outside the bound"):
        qr.check_bound("rope", wrong, ref, None, 0, 0, tile=(256, hs), bnd=bnd)


# ---- planted faults -------------------------------------------------------------------------------------------------------
FAULT_SHAPES = [(130, 264, 192, 16), (257, 8, 64, 32), (130, 320, 192, 16), (130, 132, 192, 32), (300, 320, 2048, 16)]


def _fault_outputs(c, M, N, K, rp):
    x, w, bias, ea, eb = _rounded(c)
    good = qr.linear_emulate(x, w, bias, ea, eb)
    x_drop = x.clone()
    x_drop[:, K // 2 + 1] = 0                                        # one k term never multiplied
    ea_row = ea.clone()
    ea_row[M - 2] = ea[M - 1]                                        # a row of the ragged tile clamped to row M - 1
    shifted = good.clone()
    if N >= 16:
        n0 = (N // 8 - 2) * 8
        shifted[:, n0:n0 + 8] = good[:, n0 + 8:n0 + 16]              # an 8-column chunk stored from its neighbour
    faults = {"k term dropped": qr.linear_emulate(x_drop, w, bias, ea, eb), "bias dropped": qr.linear_emulate(x, w, None, ea, eb),
              "LoRA step dropped": qr.linear_emulate(x, w, bias), "ragged row takes row M-1's ea": qr.linear_emulate(x, w, bias, ea_row, eb)}
    if N >= 16:
        faults["8-column chunk shifted by 8"] = shifted
    return good, faults


@pytest.mark.parametrize("M,N,K,rp", FAULT_SHAPES)
def test_planted_faults_break_the_bound(M, N, K, rp):
    c = qr.linear_case(M, N, K, rp)
    x, w, bias, ea, eb = _rounded(c)
    ref, S = qr.linear_ref(x, w, bias, ea, eb)
    good, faults = _fault_outputs(c, M, N, K, rp)
    qr.check_bound("good", good, ref, S, K + rp, qr.U_BF16)
    for name, y in faults.items():
        frac = qr.fraction_outside(y, ref, S, K + rp, qr.U_BF16)
        print(f"({M}, {N}, {K}) {name}: {100 * frac:.1f} % of the elements outside the bound")
        with pytest.raises(AssertionError, match="outside the bound"):
            qr.check_bound(name, y, ref, S, K + rp, qr.U_BF16)
        if name in ("bias dropped", "LoRA step dropped"):
            assert frac > 0.95                                       # a missing term shows nearly everywhere
        if name == "k term dropped":
            assert frac > (0.6 if K <= 256 else 0.2)
        if name == "ragged row takes row M-1's ea":
            wrong_rows = ((qr.f64(y) - ref).abs() > qr.bound(ref, S, K + rp, qr.U_BF16)).any(dim=1).nonzero().flatten().tolist()
            assert wrong_rows == [M - 2]


def test_the_whole_tensor_check_misses_a_dropped_bias():
    """tests/test_lora_gpu.py::test_hand_written_qlora_gemm at (2048, 2560, 2048, 16), its own input recipe (weight std 0.05,
    nn.Linear's bias <= 1 / sqrt(K) = 0.022, LoRA operands std 0.1, y of std 2.3): a result WITHOUT the bias has _rel 4.3e-3 and
    passes that test's `_rel < 1e-2` (a correct one has 2.6e-3); one without the LoRA step has 2.4e-2 and is caught, by a factor
    2.4.  The element-wise bound rejects both even here, where the bias is under one bf16 step of most elements (9 % and 55 % of
    the elements, looked at on the first 256 rows); with the recipe of qlora_ref.linear_case it is more than 95 % (above).
    This records the gap; it asks nothing of the kernels."""
    from fastmax_experiments_amd import lora
    M, N, K, rp = 2048, 2560, 2048, 16
    g = torch.Generator().manual_seed(M + N + K)
    torch.manual_seed(0)
    lin = torch.nn.Linear(K, N)
    torch.nn.init.normal_(lin.weight, std=0.05, generator=g)
    q = lora.NF4Linear.from_linear(lin)
    wd = q.dequantize(torch.bfloat16)
    x = torch.randn(M, K, generator=g).to(BF16)
    ea = (torch.randn(M, rp, generator=g) * 0.1).to(BF16)
    eb = (torch.randn(N, rp, generator=g) * 0.1).to(BF16)
    ref32 = x.float() @ wd.float().T + q.bias.float() + ea.float() @ eb.float().T
    rel = lambda a, b: float((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-30))
    no_bias = qr.linear_emulate(x, wd, None, ea, eb)
    no_lora = qr.linear_emulate(x, wd, q.bias)
    good = qr.linear_emulate(x, wd, q.bias, ea, eb)
    ref, S = qr.linear_ref(x[:256], wd, q.bias, ea[:256], eb)
    no_bias_head, no_lora_head = no_bias[:256], no_lora[:256]
    print(f"_rel: bias dropped {rel(no_bias, ref32):.2e}, LoRA step dropped {rel(no_lora, ref32):.2e}, correct "
          f"{rel(good, ref32):.2e}; outside the bound: {100 * qr.fraction_outside(no_bias_head, ref, S, K + rp, qr.U_BF16):.1f} % / "
          f"{100 * qr.fraction_outside(no_lora_head, ref, S, K + rp, qr.U_BF16):.1f} %")
    assert rel(no_bias, ref32) < 1e-2
    assert 1e-2 < rel(no_lora, ref32) < 3e-2                          # the LoRA step IS missed by that test, by a factor 2.4
    for y in (no_bias_head, no_lora_head):                            # the element-wise bound rejects both, even at these magnitudes
        with pytest.raises(AssertionError, match="outside the bound"):
            qr.check_bound("faulty", y, ref, S, K + rp, qr.U_BF16)
    qr.check_bound("correct", good[:256], ref, S, K + rp, qr.U_BF16)


def test_guarded_buffer_sees_every_kind_of_stray_write():
    for dtype in (torch.bfloat16, torch.float32):
        g = qr.Guarded2D(3, 8, 16, dtype, device="cpu")
        assert g.untouched() and g.t.shape == (3, 8) and g.t.stride(0) == 16
        with pytest.raises(AssertionError, match="unwritten"):
            g.check("y")
        g.t.zero_()
        g.check("y")
        for what, hit in (("before", lambda h: h.buf[qr.GUARD - 1:qr.GUARD].zero_()), ("past", lambda h: h.buf[-qr.GUARD:-qr.GUARD + 1].zero_()),
                          ("gap", lambda h: h.full[1, 8:9].zero_())):
            h = qr.Guarded2D(3, 8, 16, dtype, device="cpu")
            h.t.zero_()
            hit(h)
            with pytest.raises(AssertionError, match=what):
                h.check("y")
        # a NaN written over a NaN with other bits is a write too
        h = qr.Guarded2D(2, 8, 16, dtype, device="cpu")
        h.t.zero_()
        qr._bits(h.buf)[0] ^= 1
        with pytest.raises(AssertionError, match="before"):
            h.check("y")
    p = qr.padded(torch.ones(3, 8), device="cpu")
    assert p.stride(0) == 16 and float(p.sum()) == 24
