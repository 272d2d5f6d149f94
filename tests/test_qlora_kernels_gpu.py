"""The QLoRA kernels (csrc/nf4_gemm.hip, csrc/nf4_lora.hip with nf4_gemv.h, csrc/lora_thin.hip) one entry point at a time, straight
through the C ABI: every result against float64 on the operand values the kernel sees, ELEMENT BY ELEMENT within the derived bound
of tests/qlora_ref.py; every case once with contiguous operands and once with every leading dimension 8 elements wider than the
row (the two runs must give the same bits: no kernel's summation order depends on an address); every output between bands of NaN
with NaN gap columns that must come back bit for bit.  The shapes are the smallest that cross every tile edge, including the
ones the Python layers never send (N % 4, K % 64 on the few-rows entry point; RoPE tiles that span two sequences).  Each case
prints its worst |err| / bound and the element that attains it (pytest -s).  Needs an MI355X."""
import contextlib
import ctypes
import math

import pytest
import torch

import qlora_ref as qr

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from fastmax_experiments_amd import _lib
    _lib.lib()


def _L():
    from fastmax_experiments_amd import _lib
    return _lib.lib()


def _abi():
    from fastmax_experiments_amd import _lib
    return _lib


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dt(dtype):
    return _abi().BF16 if dtype == BF16 else _abi().F32


def _p(t):
    return None if t is None else t.data_ptr()


def _lay(t, pad):
    """a host operand on the device, contiguous or with a leading dimension 8 elements wider than its rows"""
    if t is None:
        return None
    return qr.padded(t.to(DEV)) if pad else t.to(DEV).contiguous()


def _done(rc, what):
    torch.cuda.synchronize()
    assert rc == 0, f"{what}: rc = {rc}"


def _report(kernel, case, worst):
    print(f"RATIO {kernel} {case}: {worst}")


def _same_bits(results, what):
    first = results[0]
    for other in results[1:]:
        assert torch.equal(qr._bits(first.contiguous()), qr._bits(other.contiguous())), f"{what}: the operands' layout changed the bits"


@contextlib.contextmanager
def _gemm_sched(value):
    L = _L()
    assert L.fastmax_hip_tune(b"gemm_sched", value) == 0
    try:
        yield
    finally:
        assert L.fastmax_hip_tune(b"gemm_sched", 0) == 0


class _Weight:
    """the frozen weight of a case as an entry point takes it: dense bf16, or NF4 codes with plain / double-quantised scales;
    `seen` = the bf16 values the matrix cores are fed"""

    def __init__(self, w, kind):
        from fastmax_experiments_amd import lora
        self.kind = kind
        if kind == "dense":
            self.seen = w.to(BF16)
            self.data, self.scales, self.nf4 = self.seen.to(DEV).contiguous(), None, 0
        else:
            packed, qs, wd = qr.quantize(w, kind == "nf4dq")
            self.seen = wd.to(BF16)
            self.host = wd
            self.qs = list(qs)
            self.qs[0] = qs[0].to(DEV)
            if qs[4] is not None:
                self.qs[4] = [qs[4][0], [qs[4][1][0].to(DEV), qs[4][1][1].to(DEV)]]
            self.data, self.scales, self.nf4 = packed.to(DEV), lora.NF4Scales(self.qs), 1

    @property
    def ref(self):
        return None if self.scales is None else self.scales.ref


# ---- 1. fastmax_hip_qlora_gemm --------------------------------------------------------------------------------------------
def _gemm(x, wt, bias, ea, eb, rp, y, M, N, K):
    rc = _L().fastmax_hip_qlora_gemm(x.data_ptr(), x.stride(0), wt.data.data_ptr(), wt.nf4, wt.ref, _p(bias), _p(ea), _p(eb), rp,
                                     y.ptr(), y.ld, M, N, K, _st())
    _done(rc, "fastmax_hip_qlora_gemm")


GEMM_CASES = ([(s, "dense", sched) for s in qr.GEMM_SHAPES for sched in (0, 12, 13, 14)]
              + [(s, "nf4", sched) for s in qr.GEMM_SHAPES for sched in (0, 14)]
              + [(qr.GEMM_DQ_SHAPE, "nf4dq", 0), (qr.GEMM_DQ_SHAPE, "nf4dq", 14), (qr.GEMM_DQ_SHAPE, "dense", 0)]
              + [(s, "nf4dq", 0) for s in qr.GEMM_SHAPES])


@pytest.mark.parametrize("shape,kind,sched", GEMM_CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{k}-sched{c}" for s, k, c in GEMM_CASES])
def test_qlora_gemm_element_by_element(shape, kind, sched):
    """bf16 in and out; dense weight under every kernel choice ("gemm_sched" 0: 128-row tiles at these sizes, 12 the same forced,
    13 the 256 x 256 kernel, 14 the plain loop), NF4 decoded in the loop with plain and double-quantised scales; rank_pad 0, 16,
    32, with and without bias"""
    M, N, K = shape
    worst_all = qr.Worst(0.0, 0, 0)
    for rp in qr.GEMM_RANKS:
        c = qr.linear_case(M, N, K, rp)
        wt = _Weight(c.w, kind)
        x = c.x.to(BF16)
        for bias in (None, c.bias):
            ref, S = qr.linear_ref(x, wt.seen, bias, c.ea, c.eb)
            runs = []
            for pad in (0, qr.PAD):
                y = qr.Guarded2D(M, N, N + pad)
                with _gemm_sched(sched):
                    _gemm(_lay(x, pad), wt, _lay(bias, 0), _lay(c.ea, 0), _lay(c.eb, 0), rp, y, M, N, K)
                y.check(f"y (ld = N + {pad})")
                worst = qr.check_bound(f"rank_pad {rp} bias {bias is not None} ld + {pad}", y.t, ref, S, K + rp, qr.U_BF16, tile=(128, 256))
                worst_all = max(worst_all, worst)
                runs.append(y.t.clone())
            _same_bits(runs, "qlora_gemm")
    _report("qlora_gemm", f"{shape} {kind} sched {sched}", worst_all)


@pytest.mark.parametrize("shape", qr.GEMM_SHAPES)
@pytest.mark.parametrize("kind,sched", [("dense", 0), ("dense", 13), ("dense", 14), ("nf4", 0)])
@pytest.mark.parametrize("rp", [16, 32])
def test_qlora_gemm_terms_one_at_a_time(shape, kind, sched, rp):
    """operands on a grid (multiples of 1/8 up to 1/2) make every partial sum exact in float32, so the expected bits do not depend
    on the order of the sum: x = 0 leaves bf16(bias + ea eb^T); ea = 0 leaves the result without the step; W = 0 without the
    step leaves bf16(bias) on every row, the ragged ones included"""
    M, N, K = shape
    c = qr.linear_case(M, N, K, rp)
    wt = _Weight(c.w, kind)
    bias = qr.exact_grid((N,), 1)
    ea, eb = qr.exact_grid((M, rp), 2).to(BF16), qr.exact_grid((N, rp), 3).to(BF16)
    x = c.x.to(BF16)

    def run(x, wt, bias, ea, eb, pad):
        y = qr.Guarded2D(M, N, N + pad)
        with _gemm_sched(sched):
            _gemm(_lay(x, pad), wt, _lay(bias, 0), _lay(ea, 0), _lay(eb, 0), rp if ea is not None else 0, y, M, N, K)
        y.check("y")
        return y.t.cpu()

    for pad in (0, qr.PAD):
        got = run(torch.zeros_like(x), wt, bias, ea, eb, pad)
        want = (bias[None, :].double() + ea.double() @ eb.double().t()).to(BF16)        # exact in float64 and in float32
        assert torch.equal(got, want), "x = 0: y != bf16(bias + ea eb^T)"
        assert torch.equal(run(x, wt, bias, torch.zeros_like(ea), c.eb, pad), run(x, wt, bias, None, None, pad)), "ea = 0 changed y"
        w0 = _Weight(torch.zeros(N, K), kind)
        got = run(x, w0, bias, None, None, pad)
        assert torch.equal(got, bias.to(BF16)[None, :].expand(M, N)), "W = 0: y != bf16(bias) on every row"


# ---- 2. fastmax_hip_nf4_linear_forward_s ------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,kern", qr.FWD_SHAPES, ids=[f"{m}x{n}x{k}-{kn}" for m, n, k, kn in qr.FWD_SHAPES])
@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("dq", [False, True], ids=["plain", "dq"])
def test_nf4_linear_forward_element_by_element(M, N, K, kern, dt, dq):
    """the 128 x 128 tile kernel at the ABI's own limits (N % 4, K % 64), the few-rows kernel (M <= 16, N % 16, K % 128) and
    M <= 16 rows falling back to the tile kernel; float32 calls round x to bf16 on the way in.  Rows must stay 16-byte aligned, so
    the tightest bf16 y for N = 132 has ldy = 136 (a contiguous one is refused: test_refusals_of_the_nf4_entry_points); the second
    run adds 8 elements to that"""
    from fastmax_experiments_amd import lora
    worst_all = qr.Worst(0.0, 0, 0)
    per16 = 16 // (2 if dt == BF16 else 4)
    ld0 = -(-N // per16) * per16                                     # the smallest leading dimension with 16-byte rows
    for rp in (0, lora.RANK_PAD):
        c = qr.linear_case(M, N, K, rp)
        wt = _Weight(c.w, "nf4dq" if dq else "nf4")
        x = c.x.to(dt)
        ead, ebd = _lay(c.ea, 0), _lay(c.eb, 0)
        for bias in (None, c.bias):
            ref, S = qr.linear_ref(x.to(BF16), wt.seen, bias, c.ea, c.eb)
            biasd = _lay(bias, 0)
            runs = []
            for pad in (0, qr.PAD):
                y = qr.Guarded2D(M, N, ld0 + pad, dt)
                xd = _lay(x, pad)
                rc = _L().fastmax_hip_nf4_linear_forward_s(xd.data_ptr(), xd.stride(0), wt.data.data_ptr(), wt.ref, _p(biasd), _p(ead), _p(ebd),
                                                           y.ptr(), y.ld, M, N, K, _dt(dt), _st())
                _done(rc, "fastmax_hip_nf4_linear_forward_s")
                y.check(f"y (ld = {ld0 + pad})")
                worst = qr.check_bound(f"{kern} rank_pad {rp} bias {bias is not None} ld + {pad}", y.t, ref, S, K + rp, qr.u_out(dt),
                                       tile=(128, 128) if kern == "tile" else (16, 16))
                worst_all = max(worst_all, worst)
                runs.append(y.t.clone())
            _same_bits(runs, "nf4_linear_forward_s")
    _report("nf4_linear_forward_s", f"{(M, N, K)} {kern} {dt} dq {dq}", worst_all)


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
def test_few_rows_with_a_bias_off_16_bytes_take_the_tile_kernel(dt):
    """the header asks no alignment of the bias: with M <= 16 and a bias 4 bytes past a 16-byte boundary the entry point sends the
    call to the tile kernel, which reads the bias four floats at a time from wherever it lies; the same function"""
    M, N, K = 3, 48, 256
    c = qr.linear_case(M, N, K, 0, seed=3)
    wt = _Weight(c.w, "nf4")
    x = c.x.to(dt)
    ref, S = qr.linear_ref(x.to(BF16), wt.seen, c.bias)
    buf = torch.zeros(N + 4, device=DEV)
    biasd = buf[1:1 + N]
    biasd.copy_(c.bias)
    assert biasd.data_ptr() % 16 == 4
    y, xd = qr.Guarded2D(M, N, N + qr.PAD, dt), _lay(x, 0)
    rc = _L().fastmax_hip_nf4_linear_forward_s(xd.data_ptr(), xd.stride(0), wt.data.data_ptr(), wt.ref, biasd.data_ptr(), None, None, y.ptr(), y.ld,
                                               M, N, K, _dt(dt), _st())
    _done(rc, "fastmax_hip_nf4_linear_forward_s")
    y.check("y")
    _report("nf4_linear_forward_s", f"{(M, N, K)} bias 4 bytes off {dt}", qr.check_bound("y", y.t, ref, S, K, qr.u_out(dt), tile=(128, 128)))


# ---- 3. fastmax_hip_nf4_linear_backward_input_s ---------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", qr.DX_SHAPES)
@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("dq", [False, True], ids=["plain", "dq"])
def test_nf4_linear_backward_input_element_by_element(M, N, K, dt, dq):
    c = qr.linear_case(M, N, K, 0)
    wt = _Weight(c.w, "nf4dq" if dq else "nf4")
    dy = torch.randn(M, N, generator=torch.Generator().manual_seed(M + N)).to(dt)
    ref, S = qr.linear_ref(dy.to(BF16), wt.seen.t())
    runs = []
    for pad in (0, qr.PAD):
        dx = qr.Guarded2D(M, K, K + pad, dt)
        dyd = _lay(dy, pad)
        rc = _L().fastmax_hip_nf4_linear_backward_input_s(dyd.data_ptr(), dyd.stride(0), wt.data.data_ptr(), wt.ref, dx.ptr(), dx.ld, M, N, K,
                                                          _dt(dt), _st())
        _done(rc, "fastmax_hip_nf4_linear_backward_input_s")
        dx.check(f"dx (ld = K + {pad})")
        worst = qr.check_bound(f"dx ld + {pad}", dx.t, ref, S, N, qr.u_out(dt), tile=(128, 128))
        runs.append(dx.t.clone())
    _same_bits(runs, "nf4_linear_backward_input_s")
    _report("nf4_linear_backward_input_s", f"{(M, N, K)} {dt} dq {dq}", worst)


# ---- 4. fastmax_hip_nf4_dequantize_s, fastmax_hip_nf4_dequantize_transposed -----------------------------------------------
@pytest.mark.parametrize("N,K", [(1, 64), (128, 192)])
@pytest.mark.parametrize("dq", [False, True], ids=["plain", "dq"])
def test_nf4_dequantize_matches_the_host_codec_bit_for_bit(N, K, dq):
    """bf16 through the 16-byte kernel (aligned `out`) and through the scalar one (`out` 8 bytes off), float32; all between bands"""
    g = torch.Generator().manual_seed(N + K)
    wt = _Weight(torch.randn(N, K, generator=g), "nf4dq" if dq else "nf4")
    n = N * K
    for dt, off in ((BF16, 0), (BF16, 4), (F32, 0)):
        out = qr.Guarded2D(1, n, n, dt, off=off)
        assert out.ptr() % 16 == 2 * off
        rc = _L().fastmax_hip_nf4_dequantize_s(wt.data.data_ptr(), wt.ref, out.ptr(), n, _dt(dt), _st())
        _done(rc, "fastmax_hip_nf4_dequantize_s")
        out.check(f"out ({dt}, {2 * off} bytes off)")
        assert torch.equal(out.t.cpu().view(N, K), wt.host.to(dt)), f"{dt}, {2 * off} bytes off: not the codec's values"


@pytest.mark.parametrize("N,K", [(64, 64), (128, 192)])
@pytest.mark.parametrize("dq", [False, True], ids=["plain", "dq"])
def test_nf4_dequantize_transposed_is_the_transpose(N, K, dq):
    g = torch.Generator().manual_seed(N + K + 1)
    wt = _Weight(torch.randn(N, K, generator=g), "nf4dq" if dq else "nf4")
    out = qr.Guarded2D(K, N, N)
    rc = _L().fastmax_hip_nf4_dequantize_transposed(wt.data.data_ptr(), wt.ref, out.ptr(), N, K, _st())
    _done(rc, "fastmax_hip_nf4_dequantize_transposed")
    out.check("out")
    assert torch.equal(out.t.cpu(), wt.host.to(BF16).t())


# ---- 5. fastmax_hip_qlora_gemm_rope ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,G,qpk,hs,rope_n,K", qr.ROPE_SHAPES, ids=["hs64-full", "hs32-partial", "hs128-full"])
@pytest.mark.parametrize("tables16", [0, 1])
@pytest.mark.parametrize("rp", [0, 16])
def test_qlora_gemm_rope_epilogue(B, T, G, qpk, hs, rope_n, K, tables16, rp):
    """256-row tiles that span two sequences (T = 130, 100): q, k, v bit-identical to fastmax_hip_qlora_gemm followed by
    fastmax_hip_rope_qkv_split (k, v at their G heads), and within the bound of the product carried through the rotation"""
    M, N, H = B * T, G * (qpk + 2) * hs, G * qpk
    c = qr.linear_case(M, N, K, rp, seed=1)
    wt = _Weight(c.w, "dense")
    x = c.x.to(BF16)
    g = torch.Generator().manual_seed(T + rope_n)
    ang = torch.rand(T, rope_n, generator=g) * 6.28
    cos, sin = ang.cos(), ang.sin()
    if tables16:                                                     # a 16-bit rope cache, handed over as float32
        cos, sin = cos.to(BF16).float(), sin.to(BF16).float()
    cosd, sind, biasd, ead, ebd = (_lay(t, 0) for t in (cos, sin, c.bias, c.ea, c.eb))
    # the two-kernel form
    y = qr.Guarded2D(M, N, N)
    _gemm(_lay(x, 0), wt, biasd, ead, ebd, rp, y, M, N, K)
    y.check("y")
    want = [qr.Guarded2D(B * H * T, hs), qr.Guarded2D(B * G * T, hs), qr.Guarded2D(B * G * T, hs)]
    rc = _L().fastmax_hip_rope_qkv_split(y.ptr(), cosd.data_ptr(), sind.data_ptr(), *(w.ptr() for w in want), B, T, G, qpk, hs, rope_n,
                                         16 * tables16, _abi().BF16, _st())
    _done(rc, "fastmax_hip_rope_qkv_split")
    # float64: the product, then the rotation
    ref_y, S = qr.linear_ref(x, wt.seen, c.bias, c.ea, c.eb)
    by = qr.bound(ref_y, S, K + rp, qr.U_BF16)
    refs = qr.split_qkv(qr.rope_apply(ref_y, cos.double(), sin.double(), T, G, qpk, hs, rope_n), T, G, qpk, hs)
    bnds = qr.split_qkv(qr.rope_bound(ref_y, by, cos, sin, T, G, qpk, hs, rope_n, bool(tables16)), T, G, qpk, hs)
    worst_all = qr.Worst(0.0, 0, 0)
    for pad in (0, qr.PAD):
        got = [qr.Guarded2D(B * H * T, hs), qr.Guarded2D(B * G * T, hs), qr.Guarded2D(B * G * T, hs)]
        xd = _lay(x, pad)
        rc = _L().fastmax_hip_qlora_gemm_rope(xd.data_ptr(), xd.stride(0), wt.data.data_ptr(), _p(biasd), _p(ead), _p(ebd), rp, cosd.data_ptr(),
                                              sind.data_ptr(), *(t.ptr() for t in got), M, N, K, T, G, qpk, hs, rope_n, tables16, _st())
        _done(rc, "fastmax_hip_qlora_gemm_rope")
        for name, a, b, r, bd in zip("qkv", got, want, refs, bnds):
            a.check(name)
            assert torch.equal(qr._bits(a.t), qr._bits(b.t)), f"{name}: not the bits of qlora_gemm + rope_qkv_split (ldx = K + {pad})"
            worst_all = max(worst_all, qr.check_bound(name, a.t, r.reshape(-1, hs), None, 0, 0, tile=(T, hs), bnd=bd.reshape(-1, hs)))
    _report("qlora_gemm_rope", f"{(B, T, G, qpk, hs, rope_n, K)} tables16 {tables16} rank_pad {rp}", worst_all)


# ---- 6. fastmax_hip_lora_down (+ _dropout) --------------------------------------------------------------------------------
def _down(x, bt, e, et, M, K, RP, drop=None):
    args = (x.data_ptr(), x.stride(0), bt.data_ptr(), bt.stride(0), e.ptr(), e.ld, None if et is None else et.ptr(), 0 if et is None else et.ld,
            M, K, RP)
    if drop is None:
        rc = _L().fastmax_hip_lora_down(*args, _st())
    else:
        rc = _L().fastmax_hip_lora_down_dropout(*args, drop[0].data_ptr(), float(drop[1]), _st())
    _done(rc, "fastmax_hip_lora_down")


@pytest.mark.parametrize("M", qr.DOWN_M)
@pytest.mark.parametrize("K", qr.DOWN_K)
@pytest.mark.parametrize("RP", qr.DOWN_RP)
def test_lora_down_element_by_element(M, K, RP):
    """16 rows per workgroup: one ragged group, one group + 1 row, nine groups with 2 rows in the last; e with lde = RP and RP + 8,
    e^T with ldet = roundup(M, 16) and 16 more: zero from column M to ldet, nothing anywhere else"""
    c = qr.linear_case(M, RP, K, 0)
    x, bt = c.x.to(BF16), c.w.to(BF16)
    ref, S = qr.linear_ref(x, bt)
    MP = (M + 15) // 16 * 16
    runs, worst = [], qr.Worst(0.0, 0, 0)
    for pad in (0, qr.PAD):
        for ldet in (MP, MP + 16):
            e = qr.Guarded2D(M, RP, RP + pad)
            et = qr.Guarded2D(RP, ldet // 16 * 16, ldet)
            _down(_lay(x, pad), _lay(bt, pad), e, et, M, K, RP)
            e.check("e")
            et.check("et")
            worst = max(worst, qr.check_bound(f"e (ld + {pad}, ldet {ldet})", e.t, ref, S, K, qr.U_BF16))
            assert torch.equal(et.t[:, :M], e.t.t()), "et[:, :M] != e^T"
            assert not et.t[:, M:].any(), "et is not zero from column M to ldet"
            runs.append(e.t.clone())
    e = qr.Guarded2D(M, RP, RP)
    _down(_lay(x, 0), _lay(bt, 0), e, None, M, K, RP)             # without the transposed copy
    e.check("e")
    runs.append(e.t.clone())
    _same_bits(runs, "lora_down")
    _report("lora_down", f"{(M, K, RP)}", worst)


def _seed():
    return torch.tensor([0x1234567, 0], dtype=torch.int32, device=DEV)


def _mask(M, K, p):
    from fastmax_experiments_amd import lora
    return lora.dropout_mask(_seed(), M, K, p).cpu()


@pytest.mark.parametrize("M,K,RP", [(17, 64, 16), (130, 192, 32)])
def test_lora_down_dropout_is_the_plain_kernel_on_the_masked_input(M, K, RP):
    """e = bf16(scale * sum(mask o x . bt)), the scale applied to the float32 sum.  p = 0.5: scale = 2 exactly, so the plain kernel
    on the bf16 matrix 2 (mask o x) -- exact -- forms the same sum and must give the same bits (tolerance 0).  p = 0.05: the scale
    (65536 / 62259) is one more float32 rounding before the bf16 one: the bound with depth K + 1 against float64."""
    c = qr.linear_case(M, RP, K, 0, seed=2)
    x, bt = c.x.to(BF16), c.w.to(BF16)
    MP = (M + 15) // 16 * 16
    from fastmax_experiments_amd import lora
    for p in (0.5, 0.05):
        mask = _mask(M, K, p)
        assert 0 < int(mask.sum()) < M * K
        scale = lora.dropout_scale(p)
        got, gott = qr.Guarded2D(M, RP, RP + qr.PAD), qr.Guarded2D(RP, MP, MP)
        _down(_lay(x, qr.PAD), _lay(bt, 0), got, gott, M, K, RP, drop=(_seed(), p))
        got.check("e")
        gott.check("et")
        assert torch.equal(gott.t[:, :M], got.t.t()) and not gott.t[:, M:].any()
        if p == 0.5:
            assert scale == 2.0
            plain = qr.Guarded2D(M, RP, RP)
            _down(_lay((x.float() * mask * 2.0).to(BF16), 0), _lay(bt, 0), plain, None, M, K, RP)
            assert torch.equal(qr._bits(got.t), qr._bits(plain.t)), "dropout p = 0.5 != the plain kernel on 2 (mask o x)"
        xm = qr.f64(x) * mask
        ref, S = (xm @ qr.f64(bt).t()) * scale, (xm.abs() @ qr.f64(bt).abs().t()) * scale
        _report("lora_down_dropout", f"{(M, K, RP)} p {p}", qr.check_bound(f"e p {p}", got.t, ref, S, K + 1, qr.U_BF16))


# ---- 7. fastmax_hip_lora_tn (+ _dropout) ----------------------------------------------------------------------------------
def _tn(et, x, out, out_dt, transpose, R, M, ncols, RP, drop=None):
    nb = _L().fastmax_hip_lora_tn_workspace(M, ncols, RP)
    assert nb > 0 and nb % 4 == 0
    ws = qr.Guarded2D(1, nb // 4, nb // 4, F32)                      # exactly the bytes asked for, between bands
    args = (et.data_ptr(), et.stride(0), x.data_ptr(), x.stride(0), out.ptr(), _dt(out_dt), transpose, R, ws.ptr(), M, ncols, RP)
    if drop is None:
        rc = _L().fastmax_hip_lora_tn(*args, _st())
    else:
        rc = _L().fastmax_hip_lora_tn_dropout(*args, drop[0].data_ptr(), float(drop[1]), _st())
    _done(rc, "fastmax_hip_lora_tn")
    ws.check("workspace", payload_written=False)
    return nb


def _tn_operands(M, ncols, RP, seed=0):
    g = torch.Generator().manual_seed(7 * M + ncols + RP + seed)
    MP = (M + 15) // 16 * 16
    et = torch.zeros(RP, MP, dtype=BF16)                              # as lora_down writes it: zero from column M on
    et[:, :M] = torch.randn(RP, M, generator=g).to(BF16)              # the rows from R on are NOT zero: they must not reach `out`
    return et, torch.randn(M, ncols, generator=g).to(BF16)


@pytest.mark.parametrize("M,ncols,R,RP", qr.TN_SHAPES)
def test_lora_tn_element_by_element(M, ncols, R, RP):
    """64-row stages, row ranges from tn_plan: M = 130 is three ranges with 2 rows in the last, M = 2049 x 64 columns 33 ranges (the
    reduce kernel's unrolled and tail loops); R < RP and R = RP, both result types, both orientations"""
    et, x = _tn_operands(M, ncols, RP)
    ref, S = qr.linear_ref(et[:R, :M], x.t())
    ceil = lambda a, b: -(-a // b)
    splits = min(ceil(1024, ncols // 64), ceil(M, 64))               # tn_plan: about 1024 workgroups, 64-row stages
    rows_per_split = ceil(ceil(M, splits), 64) * 64
    S_ = ceil(M, rows_per_split)
    assert S_ == {130: 3, 1: 1, 2049: 33}[M]
    assert _L().fastmax_hip_lora_tn_workspace(M, ncols, RP) == S_ * RP * ncols * 4
    worst_all = qr.Worst(0.0, 0, 0)
    for out_dt in (F32, BF16):
        for transpose in (0, 1):
            runs = []
            for pad in (0, qr.PAD):
                out = qr.Guarded2D(ncols, R, R, out_dt) if transpose else qr.Guarded2D(R, ncols, ncols, out_dt)
                _tn(_lay(et, pad), _lay(x, pad), out, out_dt, transpose, R, M, ncols, RP)
                out.check("out")
                got = out.t.t() if transpose else out.t
                worst_all = max(worst_all, qr.check_bound(f"{out_dt} transpose {transpose} ld + {pad}", got, ref, S, M, qr.u_out(out_dt), tile=(16, 64)))
                runs.append(got.clone())
            _same_bits(runs, "lora_tn")
    _report("lora_tn", f"{(M, ncols, R, RP)}", worst_all)


@pytest.mark.parametrize("M,ncols,R,RP", [(130, 128, 8, 16), (2049, 64, 32, 32)])
def test_lora_tn_dropout_is_the_plain_kernel_on_the_masked_input(M, ncols, R, RP):
    """out = scale * (et . (mask o x)), the scale applied by the reduce pass to the float32 total; p = 0.5: scale = 2, the plain
    kernel on 2 (mask o x) forms the doubled sums exactly: the same bits (tolerance 0)"""
    et, x = _tn_operands(M, ncols, RP, seed=1)
    mask = _mask(M, ncols, 0.5)
    for out_dt in (F32, BF16):
        got, plain = qr.Guarded2D(R, ncols, ncols, out_dt), qr.Guarded2D(R, ncols, ncols, out_dt)
        _tn(_lay(et, 0), _lay(x, qr.PAD), got, out_dt, 0, R, M, ncols, RP, drop=(_seed(), 0.5))
        _tn(_lay(et, 0), _lay((x.float() * mask * 2.0).to(BF16), 0), plain, out_dt, 0, R, M, ncols, RP)
        got.check("out")
        assert torch.equal(qr._bits(got.t), qr._bits(plain.t))


# ---- 8. fastmax_hip_lora_up (+ _dropout) ----------------------------------------------------------------------------------
def _up(y, e, bn, bn_t, bias, M, N, R, drop=None):
    args = (y.ptr(), y.ld, e.data_ptr(), e.stride(0), bn.data_ptr(), bn.stride(0), bn_t, _p(bias), M, N, R)
    if drop is None:
        rc = _L().fastmax_hip_lora_up(*args, _st())
    else:
        rc = _L().fastmax_hip_lora_up_dropout(*args, drop[0].data_ptr(), float(drop[1]), _st())
    _done(rc, "fastmax_hip_lora_up")


def _up_operands(M, N, R):
    g = torch.Generator().manual_seed(R + N + M)
    return (torch.randn(M, N, generator=g).to(BF16), torch.randn(M, R, generator=g).to(BF16),
            (torch.randn(N, R, generator=g) / math.sqrt(R)).to(BF16), torch.randn(N, generator=g))


@pytest.mark.parametrize("R", qr.UP_R)
@pytest.mark.parametrize("N", qr.UP_N)
@pytest.mark.parametrize("M", qr.UP_M)
def test_lora_up_in_place_element_by_element(R, N, M):
    """a wave owns 64 x 8 (R <= 16) or 64 x 4 columns: N = 8 is below one slab, 264 one past 256, 520 one past 512; bn as (N, R) and
    as (R, N); with and without bias; y updated in place inside a padded buffer whose gap columns keep their NaN bits"""
    y0, e, bn, bias = _up_operands(M, N, R)
    worst_all = qr.Worst(0.0, 0, 0)
    for b in (None, bias):
        ref, S = qr.linear_ref(e, bn, b)
        ref, S = ref + qr.f64(y0), S + qr.f64(y0).abs()
        runs = []
        for bn_t in (0, 1):
            for pad in (0, qr.PAD):
                y = qr.Guarded2D(M, N, N + pad).fill(y0.to(DEV))
                _up(y, _lay(e, pad), _lay(bn.t() if bn_t else bn, pad), bn_t, _lay(b, 0), M, N, R)
                y.check("y")
                worst_all = max(worst_all, qr.check_bound(f"bias {b is not None} bn_t {bn_t} ld + {pad}", y.t, ref, S, R + 2, qr.U_BF16, tile=(4, 512 if R <= 16 else 256)))
                runs.append(y.t.clone())
        _same_bits(runs, "lora_up")
    _report("lora_up", f"{(R, N, M)}", worst_all)


@pytest.mark.parametrize("R,N,M", [(8, 264, 130), (32, 520, 130), (24, 8, 1)])
def test_lora_up_dropout_against_the_mask(R, N, M):
    """y += mask o (e bn^T) * scale with the mask of fastmax_hip_lora_dropout_mask: one more product than the plain update"""
    from fastmax_experiments_amd import lora
    y0, e, bn, bias = _up_operands(M, N, R)
    for p in (0.5, 0.05):
        mask, scale = _mask(M, N, p).double(), lora.dropout_scale(p)
        ref = qr.f64(y0) + qr.f64(bias) + mask * scale * (qr.f64(e) @ qr.f64(bn).t())
        S = qr.f64(y0).abs() + qr.f64(bias).abs() + mask * scale * (qr.f64(e).abs() @ qr.f64(bn).abs().t())
        y = qr.Guarded2D(M, N, N + qr.PAD).fill(y0.to(DEV))
        _up(y, _lay(e, 0), _lay(bn, 0), 0, _lay(bias, 0), M, N, R, drop=(_seed(), p))
        y.check("y")
        _report("lora_up_dropout", f"{(R, N, M)} p {p}", qr.check_bound(f"p {p}", y.t, ref, S, R + 3, qr.U_BF16))
        # where the mask dropped, y is exactly bf16(y0 + bias)
        plain = (y0.float() + bias).to(BF16)
        assert torch.equal(y.t.cpu()[mask == 0], plain[mask == 0])


# ---- 9. fastmax_hip_lora_scatter / _backward --------------------------------------------------------------------------------
def _qkv_layer(dt):
    from fastmax_experiments_amd import lora
    torch.manual_seed(9)
    layer = lora.LoRAQKVLinear(128, (8 + 4) * 16, n_head=8, n_query_groups=2, r=4, lora_alpha=6, enable_lora=(True, False, True))
    torch.nn.init.normal_(layer.lora_B, generator=torch.Generator().manual_seed(9))
    return layer.to(dt)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_lora_scatter_is_zero_pad_times_scaling(dt):
    """a LoRAQKVLinear with the k part disabled (its columns are -1 in both rows of the map), rank 2 x 4 = 8 in RP = 16 rows,
    ldet = N + 8: exactly bf16(scaling * B) at the mapped places, zero elsewhere and in the padding rows, the gap untouched"""
    layer = _qkv_layer(dt)
    rowmap, ind, part = layer._scatter_maps()
    assert (rowmap == -1).all(dim=0).any()                             # columns no part feeds
    N, r, RP = layer.linear.out_features, layer.r, 16
    R = layer.lora_A.shape[0]
    et = qr.Guarded2D(RP, N, N + qr.PAD)
    B, rowmapd = layer.lora_B.detach().to(DEV).contiguous(), rowmap.to(DEV)
    rc = _L().fastmax_hip_lora_scatter(B.data_ptr(), _dt(dt), r, rowmapd.data_ptr(), rowmap.shape[0], float(layer.scaling), et.ptr(),
                                       et.ld, N, RP, _st())
    _done(rc, "fastmax_hip_lora_scatter")
    et.check("et")
    want = (layer._dense_rows().detach().float() * layer.scaling).t().to(BF16)        # zero_pad's scatter, float32 product, one rounding
    assert layer.scaling == 1.5 and want.shape == (R, N)
    assert torch.equal(et.t.cpu()[:R], want) and not et.t[R:].any()


@pytest.mark.parametrize("b_dt", [F32, BF16], ids=["b-f32", "b-bf16"])
@pytest.mark.parametrize("d_dt", [F32, BF16], ids=["d-f32", "d-bf16"])
def test_lora_scatter_backward_is_the_gather(b_dt, d_dt):
    layer = _qkv_layer(b_dt)
    rowmap, ind, part = layer._scatter_maps()
    N, r, RP = layer.linear.out_features, layer.r, 16
    n_rows = layer.lora_B.shape[0]
    d_et = torch.randn(RP, N, generator=torch.Generator().manual_seed(3)).to(d_dt)
    dd, indd, partd = _lay(d_et, qr.PAD), ind.to(DEV), part.to(DEV)
    db = qr.Guarded2D(n_rows, r, r, b_dt)
    rc = _L().fastmax_hip_lora_scatter_backward(dd.data_ptr(), _dt(d_dt), dd.stride(0), indd.data_ptr(), partd.data_ptr(),
                                                float(layer.scaling), db.ptr(), _dt(b_dt), n_rows, r, _st())
    _done(rc, "fastmax_hip_lora_scatter_backward")
    db.check("db")
    rows = part.long()[:, None] * r + torch.arange(r)[None, :]
    want = (d_et.float()[rows, ind.long()[:, None]] * torch.tensor(layer.scaling, dtype=F32)).to(b_dt)
    assert torch.equal(db.t.cpu(), want)


# ---- 10. refusals: one call per documented condition, rejected before any launch --------------------------------------------
def _refused(calls, outputs):
    abi = _abi()
    codes = {"shape": abi.E_BAD_SHAPE, "align": abi.E_ALIGNMENT, "null": abi.E_NULL, "dtype": abi.E_BAD_DTYPE}
    for what, want, call in calls:
        rc = call()
        torch.cuda.synchronize()
        assert rc == codes[want], f"{what}: rc = {rc}, want {codes[want]}"
        for o in outputs:
            assert o.untouched(), f"{what}: refused, but the output was written"


def test_refusals_of_the_tile_gemm():
    L, M, N, K = _L(), 16, 8, 64
    x, w = torch.zeros(M + 1, K + 8, dtype=BF16, device=DEV), torch.zeros(N + 1, K + 8, dtype=BF16, device=DEV)
    bias, ea, eb = torch.zeros(N + 8, device=DEV), torch.zeros(M, 32, dtype=BF16, device=DEV), torch.zeros(N, 32, dtype=BF16, device=DEV)
    y = qr.Guarded2D(M, N, N + 8)

    def call(xp=x.data_ptr(), ldx=K, wp=w.data_ptr(), b=None, a=None, bb=None, rp=0, yp=y.ptr(), ldy=y.ld, M=M, N=N, K=K):
        return lambda: L.fastmax_hip_qlora_gemm(xp, ldx, wp, 0, None, b, a, bb, rp, yp, ldy, M, N, K, _st())
    ok = qr.Guarded2D(M, N, N + 8)
    assert call(yp=ok.ptr())() == 0                                  # the call the refused ones differ from by one argument
    torch.cuda.synchronize()
    ok.check("y")
    _refused([("K % 64", "shape", call(K=K + 1)), ("N % 8", "shape", call(N=N + 1)), ("M = 0", "shape", call(M=0)),
              ("x 8 bytes off", "align", call(xp=x.data_ptr() + 8)), ("w 8 bytes off", "align", call(wp=w.data_ptr() + 8)),
              ("y 8 bytes off", "align", call(yp=y.ptr() + 8)), ("ldx 8 bytes off", "align", call(ldx=K + 4)),
              ("ldy 8 bytes off", "align", call(ldy=N + 4)), ("bias 4 bytes off", "align", call(b=bias.data_ptr() + 4)),
              ("ea without eb", "null", call(a=ea.data_ptr())), ("rank_pad 24", "shape", call(a=ea.data_ptr(), bb=eb.data_ptr(), rp=24)),
              ("ea 8 bytes off", "align", call(a=ea.data_ptr() + 8, bb=eb.data_ptr(), rp=16)),
              ("NF4 without scales", "null", lambda: L.fastmax_hip_qlora_gemm(x.data_ptr(), K, w.data_ptr(), 1, None, None, None, None, 0, y.ptr(), y.ld, M, N, K, _st()))],
             [y])


def test_refusals_of_the_rope_gemm():
    L = _L()
    B, T, G, qpk, hs, rn, K = 1, 16, 1, 2, 64, 32, 64
    M, N = B * T, G * (qpk + 2) * hs
    x, w = torch.zeros(M + 1, K + 8, dtype=BF16, device=DEV), torch.zeros(N + 64, K, dtype=BF16, device=DEV)
    cs = torch.zeros(T + 1, 64, device=DEV)
    q, k, v = qr.Guarded2D(B * G * qpk * T, hs), qr.Guarded2D(B * G * T, hs), qr.Guarded2D(B * G * T, hs)

    def call(xp=x.data_ptr(), ldx=K, qp=q.ptr(), M=M, N=N, K=K, T=T, hs=hs, rn=rn, qpk=qpk):
        return lambda: L.fastmax_hip_qlora_gemm_rope(xp, ldx, w.data_ptr(), None, None, None, 0, cs.data_ptr(), cs.data_ptr(), qp, k.ptr(), v.ptr(),
                                                     M, N, K, T, G, qpk, hs, rn, 0, _st())
    _refused([("K % 64", "shape", call(K=K + 1)), ("M % T", "shape", call(T=T - 1)), ("N != G (qpk + 2) hs", "shape", call(N=N + 8)),
              ("256 % hs", "shape", call(hs=96, qpk=1, N=288)), ("rope_n % 16", "shape", call(rn=rn + 8)), ("rope_n > hs", "shape", call(rn=hs + 16)),
              ("x 8 bytes off", "align", call(xp=x.data_ptr() + 8)), ("q 8 bytes off", "align", call(qp=q.ptr() + 8)),
              ("ldx 8 bytes off", "align", call(ldx=K + 4))], [q, k, v])


def test_refusals_of_the_nf4_entry_points():
    L, abi = _L(), _abi()
    M, N, K = 4, 64, 128
    wt = _Weight(torch.randn(N, K + 64, generator=torch.Generator().manual_seed(0)), "nf4")
    x = torch.zeros(M + 1, max(N, K) + 8, dtype=F32, device=DEV)
    ea = torch.zeros(M, 32, dtype=BF16, device=DEV)
    y = qr.Guarded2D(M, max(N, K), max(N, K) + 8, F32)
    wq = wt.data.data_ptr()

    def fwd(xp=x.data_ptr(), ldx=K, w=wq, sc=wt.ref, a=None, yp=y.ptr(), ldy=y.ld, N=N, K=K, dt=abi.BF16):
        return lambda: L.fastmax_hip_nf4_linear_forward_s(xp, ldx, w, sc, None, a, None, yp, ldy, M, N, K, dt, _st())

    def bwd(gp=x.data_ptr(), ldg=N, w=wq, dxp=y.ptr(), ldd=y.ld, N=N, K=K, dt=abi.BF16):
        return lambda: L.fastmax_hip_nf4_linear_backward_input_s(gp, ldg, w, wt.ref, dxp, ldd, M, N, K, dt, _st())
    _refused([("forward K % 64", "shape", fwd(K=K + 1)), ("forward N % 4", "shape", fwd(N=N + 1)), ("forward x 8 bytes off", "align", fwd(xp=x.data_ptr() + 8)),
              ("forward ldx 2 bytes off (bf16)", "align", fwd(ldx=K + 1)), ("forward ldx 4 bytes off (f32)", "align", fwd(ldx=K + 1, dt=abi.F32)),
              ("forward ldy", "align", fwd(ldy=y.ld + 1)),
              ("forward contiguous bf16 y, N % 8 = 4", "align", fwd(N=N + 4, ldy=N + 4)), ("forward y 8 bytes off", "align", fwd(yp=y.ptr() + 8)),
              ("forward codes 8 bytes off", "align", fwd(w=wq + 8)), ("forward ea without eb", "null", fwd(a=ea.data_ptr())),
              ("forward without scales", "null", fwd(sc=None)), ("forward f16", "dtype", fwd(dt=abi.F16)),
              ("backward K % 128", "shape", bwd(K=K + 64)), ("backward K + 1", "shape", bwd(K=K + 1)), ("backward N % 64", "shape", bwd(N=N + 1)),
              ("backward dy 8 bytes off", "align", bwd(gp=x.data_ptr() + 8)), ("backward lddy", "align", bwd(ldg=N + 1)),
              ("backward lddx", "align", bwd(ldd=y.ld + 1)), ("backward dx 8 bytes off", "align", bwd(dxp=y.ptr() + 8)), ("backward f16", "dtype", bwd(dt=abi.F16)),
              ("dequantize n % 64", "shape", lambda: L.fastmax_hip_nf4_dequantize_s(wq, wt.ref, y.ptr(), 65, abi.BF16, _st())),
              ("dequantize n = 0", "shape", lambda: L.fastmax_hip_nf4_dequantize_s(wq, wt.ref, y.ptr(), 0, abi.BF16, _st())),
              ("dequantize f16", "dtype", lambda: L.fastmax_hip_nf4_dequantize_s(wq, wt.ref, y.ptr(), 64, abi.F16, _st())),
              ("dequantize without scales", "null", lambda: L.fastmax_hip_nf4_dequantize_s(wq, None, y.ptr(), 64, abi.BF16, _st())),
              ("transposed N % 64", "shape", lambda: L.fastmax_hip_nf4_dequantize_transposed(wq, wt.ref, y.ptr(), 65, 64, _st())),
              ("transposed K % 64", "shape", lambda: L.fastmax_hip_nf4_dequantize_transposed(wq, wt.ref, y.ptr(), 64, 65, _st())),
              ("transposed out 8 bytes off", "align", lambda: L.fastmax_hip_nf4_dequantize_transposed(wq, wt.ref, y.ptr() + 8, 64, 64, _st()))], [y])


def test_refusals_of_the_rank_r_kernels():
    """lora_down / lora_tn / lora_up report a misaligned operand as a shape error: that is the code they have always returned"""
    L, abi = _L(), _abi()
    M, K, RP, N = 17, 64, 16, 64
    MP = 32
    x = torch.zeros(M + 1, K + 8, dtype=BF16, device=DEV)
    bt = torch.zeros(32, K + 8, dtype=BF16, device=DEV)
    e, et = qr.Guarded2D(M, RP, RP + 8), qr.Guarded2D(RP, MP, MP + 16)
    out, ws = qr.Guarded2D(RP, N, N, F32), qr.Guarded2D(1, 4 * RP * N, 4 * RP * N, F32)
    y = qr.Guarded2D(M, N, N + 8)

    def down(xp=x.data_ptr(), ldx=K, ldbt=K, lde=e.ld, ldet=et.ld, K=K, RP=RP, M=M):
        return lambda: L.fastmax_hip_lora_down(xp, ldx, bt.data_ptr(), ldbt, e.ptr(), lde, et.ptr(), ldet, M, K, RP, _st())

    def tn(etp=et.ptr(), ldet=et.ld, ldx=N + 8, dt=abi.F32, R=RP, ncols=N, RP=RP):
        return lambda: L.fastmax_hip_lora_tn(etp, ldet, x.data_ptr(), ldx, out.ptr(), dt, 0, R, ws.ptr(), M, ncols, RP, _st())

    def up(yp=y.ptr(), ldy=y.ld, lde=RP, ldb=RP, N=N, R=RP, t=0):
        return lambda: L.fastmax_hip_lora_up(yp, ldy, x.data_ptr(), lde, bt.data_ptr(), ldb, t, None, M, N, R, _st())
    assert L.fastmax_hip_lora_tn_workspace(M, N + 1, RP) == -1 and L.fastmax_hip_lora_tn_workspace(M, N, 24) == -1
    assert L.fastmax_hip_lora_tn_workspace(0, N, RP) == -1
    _refused([("down K % 64", "shape", down(K=K + 1)), ("down RP 24", "shape", down(RP=24)), ("down lde < RP", "shape", down(lde=RP - 1)),
              ("down ldx < K", "shape", down(ldx=K - 8)), ("down ldbt < K", "shape", down(ldbt=K - 8)), ("down ldet < roundup(M, 16)", "shape", down(ldet=MP - 1)),
              ("down x 8 bytes off", "shape", down(xp=x.data_ptr() + 8)), ("down ldx 8 bytes off", "shape", down(ldx=K + 4)), ("down M = 0", "shape", down(M=0)),
              ("tn ncols % 64", "shape", tn(ncols=N + 1)), ("tn RP 24", "shape", tn(RP=24, R=8)), ("tn R = 0", "shape", tn(R=0)), ("tn R > RP", "shape", tn(R=RP + 1)),
              ("tn ldx < ncols", "shape", tn(ldx=N - 8)), ("tn f16", "dtype", tn(dt=abi.F16)), ("tn ldet < roundup(M, 16)", "shape", tn(ldet=MP - 4)),
              ("tn ldet 2 bytes off", "shape", tn(ldet=MP + 1)), ("tn et 2 bytes off", "shape", tn(etp=et.ptr() + 2)), ("tn ldx 8 bytes off", "shape", tn(ldx=N + 4)),
              ("up N % 8", "shape", up(N=N + 1)), ("up ldy < N", "shape", up(ldy=N - 8)), ("up lde < R", "shape", up(lde=RP - 8)), ("up ldb < R", "shape", up(ldb=RP - 8)),
              ("up ldb < N (transposed)", "shape", up(ldb=N - 8, t=1)), ("up R 12", "shape", up(R=12, lde=16, ldb=16)), ("up y 8 bytes off", "shape", up(yp=y.ptr() + 8)),
              ("up ldy 8 bytes off", "shape", up(ldy=N + 4))], [e, et, out, ws, y])


def test_refusals_of_the_scatter():
    L, abi = _L(), _abi()
    N, r, RP = 64, 8, 16
    b, rowmap = torch.zeros(N, r, device=DEV), torch.zeros(2, N, dtype=torch.int32, device=DEV)
    et, db = qr.Guarded2D(RP, N, N + 8), qr.Guarded2D(N, r, r, F32)

    def sc(dt=abi.F32, r=r, parts=2, ldet=et.ld, N=N):
        return lambda: L.fastmax_hip_lora_scatter(b.data_ptr(), dt, r, rowmap.data_ptr(), parts, 1.0, et.ptr(), ldet, N, RP, _st())

    def scb(dt=abi.F32, bdt=abi.F32, n_rows=N, r=r):
        return lambda: L.fastmax_hip_lora_scatter_backward(et.ptr(), dt, et.ld, rowmap.data_ptr(), rowmap.data_ptr(), 1.0, db.ptr(), bdt, n_rows, r, _st())
    _refused([("scatter n_parts r > RP", "shape", sc(parts=3)), ("scatter ldet < N", "shape", sc(ldet=N - 1)), ("scatter r = 0", "shape", sc(r=0)),
              ("scatter f16", "dtype", sc(dt=abi.F16)), ("scatter without a map", "null", lambda: L.fastmax_hip_lora_scatter(b.data_ptr(), abi.F32, r, None, 2, 1.0, et.ptr(), et.ld, N, RP, _st())),
              ("backward n_rows = 0", "shape", scb(n_rows=0)), ("backward r = 0", "shape", scb(r=0)), ("backward d f16", "dtype", scb(dt=abi.F16)),
              ("backward b f16", "dtype", scb(bdt=abi.F16))], [et, db])
