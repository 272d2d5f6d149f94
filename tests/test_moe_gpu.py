"""The mixture-of-experts MLP on an MI355X (csrc/moe.hip, fastmax_experiments_amd/moe.py) against moe_ref.py:

1. route: the fixtures' stored routers and synthetic ones over both launch shapes (up to 256 tokens: one launch; above: three),
   one expert taking every token, exact ties across the k-th place, NaN entries, a strided router: expert, offsets, row_of and
   slot_of exactly moe_ref's, prob32 within 4 float32 ulp of the float64 softmax, prob within 1 ulp of the dtype, two calls with
   identical bits;
2. gather bitwise a fancy index, combine bitwise moe_ref fed the kernel's own prob: the 16-byte piece path, the element path
   (C = 20, and C = 64 off a 16-byte boundary), a strided x, three dtypes, k = 3;
3. the backward kernels one by one against their exact forms, within the bounds their number formats give (stated at each);
4. fixtures through the module with kernels on: every gradient's error against moe_ref's exact gradients at most 4 x the error of
   the fixture's own (reference) gradient + 2^-(mantissa bits);
5. the module, kernels on against off on the same device: dense in bf16 / f32 and after quantize_base; one device-to-host copy;
6. block level: eager generate() through a stack of two MoE blocks gives the same tokens with kernels on and off at temperature
   0, and GraphedDecoder refuses the stack.

Ratios measured for 4. and 5. are recorded in profiles/r17_moe.md."""
import numpy as np
import pytest
import torch

import moe_ref
from block_ref import ulp_err
from conftest import golden_names, load_golden

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
FIXTURES = golden_names("moe_")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from fastmax_experiments_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _np(t):
    return t.detach().float().cpu().numpy() if t.is_floating_point() else t.detach().cpu().numpy()


def _randn(shape, seed, dt, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(DT[dt]).cuda()


# ---- 1. route ------------------------------------------------------------------------------------------------------------------
def _check_route(router, k, dt):
    """router: a device tensor (M, E) of dtype dt, any row stride"""
    from fastmax_experiments_amd import moe
    got = moe.route(router, k)
    again = moe.route(router, k)
    for a, b in zip(got, again):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "two calls differ"
    expert, prob, prob32, offsets, row_of, slot_of = got
    assert prob.dtype == DT[dt] and prob32.dtype == torch.float32
    assert all(t.dtype == torch.int32 for t in (expert, offsets, row_of, slot_of))
    ref = moe_ref.route(_np(router), k, dt)
    assert np.array_equal(_np(expert), ref["expert"])
    assert np.array_equal(_np(offsets), ref["offsets"])
    assert np.array_equal(_np(row_of), ref["row_of"])
    assert np.array_equal(_np(slot_of), ref["slot_of"])
    nan = np.isnan(ref["prob32"])
    assert np.array_equal(np.isnan(_np(prob32)), nan) and np.array_equal(np.isnan(_np(prob)), nan)
    if not nan.all():
        ok = ~nan
        assert ulp_err(_np(prob32).astype(np.float64)[ok], ref["prob32"][ok], "f32") <= 4.0
        assert ulp_err(_np(prob)[ok], ref["prob32"][ok], dt) <= 1.0
    return got


@pytest.mark.parametrize("name", FIXTURES)
def test_route_on_the_fixtures_routers(name):
    d, m = load_golden(name)
    router = torch.from_numpy(d["router"]).to(DT[m["dtype"]]).cuda()
    _check_route(router, m["n_expert_per_token"], m["dtype"])


@pytest.mark.parametrize("E, k", [(8, 2), (6, 3), (2, 2), (64, 8)])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 257, 1031])
def test_route_on_synthetic_routers(M, E, k):
    dt = ("bf16", "f32", "f16")[(M + E) % 3]
    _check_route(_randn((M, E), 100 * M + E, dt, 2.0), k, dt)


def test_route_when_one_expert_takes_every_token():
    router = _randn((300, 8), 7, "bf16")
    router[:, 5] += 50
    expert, _, prob32, offsets, row_of, _ = _check_route(router, 1, "bf16")
    assert _np(offsets).tolist() == [0] * 6 + [300] * 3
    assert np.array_equal(_np(row_of), np.arange(300)) and (_np(expert) == 5).all() and (_np(prob32) == 1.0).all()
    # with k = 2 the second choice spreads; the first expert still holds all 300 tokens in order
    _, _, _, offsets, row_of, _ = _check_route(router, 2, "bf16")
    o = _np(offsets)
    assert o[6] - o[5] == 300 and np.array_equal(_np(row_of)[o[5]:o[6]], np.arange(300))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_route_breaks_exact_ties_towards_the_lowest_index(dt):
    g = torch.Generator().manual_seed(11)
    router = torch.randint(0, 3, (517, 8), generator=g).to(DT[dt]).cuda()          # three distinct values: ties in every row
    router[5] = 1.0                                                                 # a row of eight equal entries
    router[6, 3] = -0.0
    got = _check_route(router, 3, dt)
    assert _np(got[0])[5].tolist() == [0, 1, 2]


def test_route_ranks_nan_above_every_number():
    router = _randn((70, 6), 13, "f32")
    router[3, 4] = float("nan")
    router[9, 0] = float("nan")
    router[9, 5] = float("inf")
    router[20, 2] = float("-inf")
    expert = _np(_check_route(router, 2, "f32")[0])
    assert 4 in expert[3] and expert[9].tolist() == [0, 5] and 2 not in expert[20]


def test_route_takes_a_strided_router():
    wide = _randn((261, 24), 17, "f16")
    _check_route(wide[:, 5:13], 2, "f16")               # row stride 24, rows off any 16-byte boundary
    _check_route(wide[:, :6], 3, "f16")


# ---- 2. gather and combine -------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.uint8)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("C, x_view", [(64, "dense"), (64, "strided"), (64, "offset"), (20, "dense"), (20, "strided")])
def test_gather_and_combine_are_bitwise_the_reference(C, x_view, dt):
    from fastmax_experiments_amd import moe
    M, E, k = 70, 6, 3
    router = _randn((M, E), 23, dt)
    _, prob, _, offsets, row_of, slot_of = moe.route(router, k)
    wide = _randn((M * k, C + 16), 29 + C, dt)              # rows of C + 16 elements: whole 16-byte pieces in every dtype
    view = {"dense": lambda w: w[:, :C].contiguous(), "strided": lambda w: w[:, :C], "offset": lambda w: w[:, 1:C + 1]}[x_view]
    x = view(wide[:M])
    xs = moe.gather(x, row_of)
    assert xs.shape == (M * k, C) and torch.equal(_bits(xs), _bits(x[row_of.long()]))
    ys = view(wide)
    y = moe.combine(ys, prob, slot_of)
    want = moe_ref.combine(_np(ys), _np(prob), _np(slot_of), dt)
    assert y.shape == (M, C) and y.dtype == DT[dt]
    assert np.array_equal(_np(y).astype(np.float64), want)


def test_gather_moves_nan_payloads_and_signed_zeros_untouched():
    from fastmax_experiments_amd import moe
    words = np.array([[0x7FC1, 0xFFFF, 0x8000, 0x0001] * 4, [0x7F81, 0x0000, 0x7F80, 0xFF80] * 4], dtype=np.uint16)
    x = torch.from_numpy(words.view(np.int16)).view(torch.bfloat16).cuda()
    row_of = torch.tensor([1, 0, 0, 1], dtype=torch.int32, device="cuda")
    assert torch.equal(_bits(moe.gather(x, row_of)), _bits(x[row_of.long()]))
    assert torch.equal(_bits(moe.gather(x[:, :5], row_of)), _bits(x[:, :5][row_of.long()]))


# ---- 3. the backward kernels, one by one ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("C", [64, 20, 1100])
def test_backward_kernels_against_their_exact_forms(C, dt):
    """each output is float32 arithmetic on values of the dtype, rounded ONCE to the dtype: half a unit in the last place, i.e.
    2^-(mantissa bits + 1) of the value, which the bounds below double to 2^-(mantissa bits).  The sums add what float32
    recursive summation of n terms can lose, n 2^-24 sum |terms| (n = C for dprob, k for dx and for the softmax's dot)."""
    from fastmax_experiments_amd import moe
    M, E, k = 70, 8, 3
    eps = moe_ref.eps(dt)
    expert, prob, prob32, _, _, slot_of = moe.route(_randn((M, E), 31, dt), k)
    dy, ys = _randn((M, C), 37, dt), _randn((M * k, C), 41, dt)
    slots = _np(slot_of)
    # combine backward
    dys, dprob = moe.combine_backward(dy, ys, prob, slot_of)
    dys_x, dprob_x = moe_ref.combine_backward(_np(dy), _np(ys), _np(prob), slots)
    assert moe_ref.rel_to_max(_np(dys), dys_x) <= eps
    terms = np.abs(_np(dy).astype(np.float64)[:, None, :] * _np(ys).astype(np.float64)[slots]).sum(-1)
    assert moe_ref.rel_to_max(_np(dprob), dprob_x) <= eps + C * 2.0 ** -24 * terms.max() / np.abs(dprob_x).max()
    again = moe.combine_backward(dy, ys, prob, slot_of)
    assert torch.equal(_bits(again[0]), _bits(dys)) and torch.equal(_bits(again[1]), _bits(dprob))
    # gather backward
    dx = moe.gather_backward(ys, slot_of)
    dx_x = moe_ref.gather_backward(_np(ys), slots)
    assert moe_ref.rel_to_max(_np(dx), dx_x) <= eps + k * 2.0 ** -24 * k * np.abs(_np(ys)).max() / np.abs(dx_x).max()
    # route backward
    g = _randn((M, k), 43, dt)
    dr = moe.route_backward(g, prob32, expert, E)
    dr_x = moe_ref.route_backward(_np(g), _np(prob32).astype(np.float64), _np(expert), E)
    assert dr.shape == (M, E) and moe_ref.rel_to_max(_np(dr), dr_x) <= eps + (k + 3) * 2.0 ** -24 * np.abs(_np(g)).max() / np.abs(dr_x).max()
    idle = np.ones((M, E), bool)
    np.put_along_axis(idle, _np(expert).astype(np.int64), False, axis=1)
    assert not _np(dr)[idle].any() and _np(dr)[~idle].all()                 # zero exactly where no expert was selected


# ---- 4., 5. the module -----------------------------------------------------------------------------------------------------------
def _weights(moe):
    """[(fc_1, fc_2, proj)] as float64 numpy, dequantized where the base is NF4"""
    from fastmax_experiments_amd.lora import NF4Linear
    def w(lin):
        base = lin.linear
        t = base.dequantize(torch.float32) if isinstance(base, NF4Linear) else base.weight
        return t.detach().double().cpu().numpy()
    return [tuple(w(getattr(e, n)) for n in ("fc_1", "fc_2", "proj")) for e in moe.experts]


def _run(moe, x, gy, fused):
    """-> (y, router the gate produced, dx, {name: grad}) as float64 numpy"""
    moe.fused_neighbours = fused
    seen = {}
    hook = moe.gate.register_forward_hook(lambda m, inp, out: seen.__setitem__("router", out.detach()))
    for p in moe.parameters():
        p.grad = None
    xr = x.clone().requires_grad_(True)
    y = moe(xr)
    y.backward(gy)
    hook.remove()
    grads = {n: _np(p.grad).astype(np.float64) for n, p in moe.named_parameters() if p.grad is not None}
    return _np(y).astype(np.float64), _np(seen["router"]).astype(np.float64), _np(xr.grad).astype(np.float64), grads


def _exact(moe, x, gy, router):
    """moe_ref's exact y over the router a run saw, and the exact gradients at that run's selection"""
    M, C = x.numel() // x.shape[-1], x.shape[-1]
    experts, k = _weights(moe), moe.n_expert_per_token
    x64, gy64 = _np(x).astype(np.float64).reshape(M, C), _np(gy).astype(np.float64).reshape(M, C)
    y, _, _ = moe_ref.moe_forward(x64, router, experts, k, "f32", exact=True)
    gate = moe.gate.linear.weight.detach().double().cpu().numpy()
    dx, dgate, dexp = moe_ref.moe_backward(x64, gate, experts, k, gy64, select_from=router)
    grads = {"gate.linear.weight": dgate}
    for e, g3 in enumerate(dexp):
        for n, g in zip(("fc_1", "fc_2", "proj"), g3):
            grads[f"experts.{e}.{n}.linear.weight"] = g
    return y, dx, grads


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_gradients_with_kernels_on(name):
    from test_moe_cpu import _module
    d, m = load_golden(name)
    dt, M, C = m["dtype"], m["rows"], m["n_embd"]
    moe = _module(d, m).cuda()
    x, gy = (torch.from_numpy(d[n]).to(DT[dt]).cuda() for n in ("x", "gy"))
    y, router, dx, grads = _run(moe, x, gy, True)
    assert np.array_equal(moe_ref.select(router, m["n_expert_per_token"]), moe_ref.select(d["router"], m["n_expert_per_token"]))
    y_x, dx_x, grads_x = _exact(moe, x, gy, router)
    eps = moe_ref.eps(dt)
    rows = [("dx", dx.reshape(M, C), d["dx"].reshape(M, C), dx_x)]
    for n, gx in grads_x.items():
        if np.abs(gx).max() == 0.0:                       # an expert without tokens: not called, no gradient
            assert n not in grads or not grads[n].any()
            continue
        rows.append((n, grads[n], d["d_" + n.replace(".linear", "").replace(".", "_")], gx))
    worst = 0.0
    for n, got, fixture, exact in rows:
        err, base = moe_ref.rel_to_max(got, exact), moe_ref.rel_to_max(fixture, exact)
        worst = max(worst, err / base)
        assert err <= 4 * base + eps, (n, err, base)
    print(f"[moe] {name}: worst gradient error / the reference gradient's error = {worst:.3f}")         # shown with -s


MODULE_CASES = [("bf16", 64, 128, False), ("f32", 64, 128, False), ("bf16", 128, 128, True)]


@pytest.mark.parametrize("dt, n_embd, inter, quantized", MODULE_CASES, ids=["bf16", "f32", "bf16-nf4"])
def test_module_kernels_on_against_off(dt, n_embd, inter, quantized, monkeypatch):
    from fastmax_experiments_amd import moe as moe_mod
    M, E, k = 70, 8, 2
    torch.manual_seed(3)
    moe = moe_mod.LLaMAMoE(n_embd, inter, E, k).to(DT[dt])
    if quantized:
        moe.quantize_base()
    moe = moe.cuda()
    x, gy = _randn((2, M // 2, n_embd), 51, dt, 1.5), _randn((2, M // 2, n_embd), 53, dt)
    reads = []
    real = moe_mod._read_offsets
    monkeypatch.setattr(moe_mod, "_read_offsets", lambda offsets: reads.append(offsets.numel()) or real(offsets))
    on = _run(moe, x, gy, True)
    assert reads == [E + 1], "the forward pass reads the E + 1 offsets back once; the backward pass reads nothing"
    off = _run(moe, x, gy, False)
    assert reads == [E + 1]
    eps = moe_ref.eps(dt)
    ratios = {}
    errs = {}
    for tag, (y, router, dx, grads) in (("on", on), ("off", off)):
        y_x, dx_x, grads_x = _exact(moe, x, gy, router)
        errs[tag] = {"y": moe_ref.rel_to_max(y.reshape(M, n_embd), y_x), "dx": moe_ref.rel_to_max(dx.reshape(M, n_embd), dx_x)}
        for n, g in grads.items():
            errs[tag][n] = moe_ref.rel_to_max(g, grads_x[n])
    assert set(errs["on"]) == set(errs["off"])
    assert errs["on"]["y"] <= 1.5 * errs["off"]["y"] + eps, (errs["on"]["y"], errs["off"]["y"])
    for n in errs["on"]:
        if n != "y":
            assert errs["on"][n] <= 4 * errs["off"][n] + eps, (n, errs["on"][n], errs["off"][n])
        ratios[n] = errs["on"][n] / errs["off"][n]
    print(f"[moe] module {dt}{' nf4' if quantized else ''}: y on/off = {errs['on']['y']:.3e} / {errs['off']['y']:.3e}; "
          f"worst gradient error on / off = {max(v for n, v in ratios.items() if n != 'y'):.3f}")


# ---- 6. block level ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stack():
    from fastmax_experiments_amd.attention_block import build_rope_cache
    from fastmax_experiments_amd.block import Block, BlockStack
    from fastmax_experiments_amd.generate import NextTokenHead
    torch.manual_seed(8)
    blocks = BlockStack([Block(n_embd=64, n_head=4, intermediate_size=96, mlp_class="LLaMAMoE", n_expert=4, n_expert_per_token=2)
                         for _ in range(2)]).cuda().eval()
    head = NextTokenHead(64, 97).cuda().eval()
    wte = torch.randn(97, 64).cuda()
    cos, sin = build_rope_cache(16, blocks.blocks[0].attn.rope_n_elem, device="cuda")
    prompt = torch.randint(0, 97, (2, 5), generator=torch.Generator().manual_seed(9)).cuda()
    return dict(blocks=blocks, head=head, wte=wte, cos=cos, sin=sin, prompt=prompt)


def _states():
    from fastmax_experiments_amd.decode import FastmaxDecodeState
    return [FastmaxDecodeState(2, 4, 16, "cuda", p=2, n_query_groups=4) for _ in range(2)]


def test_generate_through_moe_blocks_gives_the_same_tokens_with_kernels_on_and_off(stack):
    from fastmax_experiments_amd.generate import generate
    tokens = {}
    for fused in (True, False):
        for blk in stack["blocks"].blocks:
            blk.mlp.fused_neighbours = fused
        with torch.no_grad():
            tokens[fused] = generate(stack["wte"], stack["blocks"], stack["head"], _states(), stack["prompt"], 11, cos=stack["cos"],
                                     sin=stack["sin"], temperature=0.0)
    for blk in stack["blocks"].blocks:
        blk.mlp.fused_neighbours = True
    assert tokens[True].shape == (2, 11) and torch.equal(tokens[True][:, :5], stack["prompt"])
    assert torch.equal(tokens[True], tokens[False])


def test_graphed_decoder_refuses_moe_blocks(stack):
    from fastmax_experiments_amd.generate import GraphedDecoder
    with pytest.raises(NotImplementedError, match="row counts"):
        GraphedDecoder(stack["wte"], stack["blocks"], stack["head"], _states(), cos=stack["cos"], sin=stack["sin"], max_len=11)
