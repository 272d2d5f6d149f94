"""The decode-size expert kernels on device-side row counts, on an MI355X (csrc/moe_decode.hip, moe.experts_up / experts_down,
``LLaMAMoE.device_routed``, ``GraphedDecoder`` on Mixtral blocks).  Every comparison is ``torch.equal`` against kernels that were
there before: the experts' own modules (the few-rows NF4 product and the gated activation) run by run, the module's eager route,
the eager generation loop.  No tolerance anywhere.

1. kernel level: hand-made routers choose the runs; h and ys start as NaN, so equality also proves every slot written;
2. module level: ``device_routed`` on equals off at M = 1, 2, 16 with ``_read_offsets`` forbidden; M = 17 and a call that needs a
   gradient take the old route (one read);
3. capture: a recorded ``moe(x)`` replayed on rows that route to other experts; the table cannot be built inside a capture;
4. generation: eager with the switch on and off, ``GraphedDecoder`` with it on, a second prompt through the same graph;
5. what ``GraphedDecoder`` still refuses.

Widths n_embd / intermediate: 128/128 (one K block: waves 1 to 3 idle), 256/128 (two), 640/384 (five and three: the unpaired tail,
an idle wave in ``down``), 1152/128 (nine: the paired loop plus the tail)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f32": torch.float32}
WIDTHS = [(128, 128), (256, 128), (640, 384), (1152, 128)]
# (E, k, the experts of each token): the runs the kernels see
LAYOUTS = {
    "all 16 tokens on the same two experts": (8, 2, [(1, 4)] * 16),
    "one token": (8, 2, [(6, 2)]),
    "five tokens, expert 3 with one row, experts 2 and 6 with none": (8, 2, [(0, 1), (0, 3), (4, 5), (1, 7), (5, 7)]),
    "k = 1": (8, 1, [(7,), (0,), (7,), (3,), (0,), (0,), (5,)]),
    "k = 2, sixteen tokens spread": (8, 2, [(t % 8, (t * 3 + 1) % 8 if (t * 3 + 1) % 8 != t % 8 else (t + 2) % 8) for t in range(16)]),
    "k = 3 of 6": (6, 3, [(0, 1, 2), (3, 4, 5), (0, 2, 4), (1, 2, 5), (0, 1, 5), (2, 3, 4), (0, 4, 5), (1, 3, 5), (0, 2, 3), (2, 4, 5), (1, 2, 3)]),
}


def _router(E, chosen, dtype):
    """a router whose top-k of row t is chosen[t]: distinct values above a floor no other entry reaches"""
    r = torch.full((len(chosen), E), -4.0)
    for t, experts in enumerate(chosen):
        for j, e in enumerate(experts):
            r[t, e] = 1.0 + 0.25 * j + 0.125 * (t % 3)
    return r.to(dtype).cuda()


@functools.lru_cache(maxsize=None)
def _layer(n_embd, inter, dt, double_quant=False, bias=False, E=8, k=2, seed=5):
    from fastmax_experiments_amd.moe import LLaMAMoE
    torch.manual_seed(seed)
    layer = LLaMAMoE(n_embd, inter, E, k, bias=bias).to(DT[dt])
    if bias:
        for expert in layer.experts:                                          # biases that matter next to the products
            for lin in (expert.fc_1, expert.fc_2, expert.proj):
                torch.nn.init.normal_(lin.linear.bias, std=0.5)
    return layer.quantize_base(double_quant).cuda().eval()


def _x(M, C, dt, seed, scale=1.5):
    return (torch.randn(M, C, generator=torch.Generator().manual_seed(seed)) * scale).to(DT[dt]).cuda()


# ---- 1. kernel level ---------------------------------------------------------------------------------------------------------
def _check_kernels(layer, x, dt, layouts=LAYOUTS):
    """experts_up / experts_down on every layout against the experts' own modules run by run, bit for bit"""
    from fastmax_experiments_amd import moe
    from fastmax_experiments_amd.block import gated_act
    C, I = layer.n_embd, layer.intermediate_size
    seen = set()
    for name, (E, k, chosen) in layouts.items():
        M = len(chosen)
        xm = x[:M]
        expert, _, _, offsets, row_of, _ = moe.route(_router(E, chosen, DT[dt]), k)
        assert expert.tolist() == [sorted(c) for c in chosen], name
        table, keep = moe.expert_table(layer.experts[:E])
        h = torch.full((M * k, I), float("nan"), dtype=DT[dt], device="cuda")
        ys = torch.full((M * k, C), float("nan"), dtype=DT[dt], device="cuda")
        assert moe.experts_up(xm, table, offsets, row_of, k, I, out=h) is h
        assert moe.experts_down(h, table, offsets, k, C, out=ys) is ys
        bounds, rows = offsets.tolist(), row_of.long()
        assert bounds[0] == 0 and bounds[-1] == M * k
        with torch.no_grad():
            for e in range(E):
                lo, hi = bounds[e], bounds[e + 1]
                seen.add(hi - lo)
                if hi == lo:
                    continue
                ex, xr = layer.experts[e], xm[rows[lo:hi]]
                assert torch.equal(h[lo:hi], gated_act(ex.fc_1(xr), ex.fc_2(xr), "silu")), (name, e, "h")
                assert torch.equal(ys[lo:hi], ex(xr)), (name, e, "ys")
        assert not torch.isnan(h).any() and not torch.isnan(ys).any(), name
        del keep
    return seen


@pytest.mark.parametrize("double_quant", [False, True], ids=["nf4", "nf4-dq"])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("n_embd, inter", WIDTHS)
def test_the_expert_kernels_give_the_experts_own_bits_on_every_run_layout(n_embd, inter, dt, double_quant):
    layer = _layer(n_embd, inter, dt, double_quant)
    assert layer.experts[0].fc_1.linear.double_quant == double_quant
    seen = _check_kernels(layer, _x(16, n_embd, dt, 11), dt)
    assert {0, 1, 16} <= seen, "the layouts should hold an empty run, a single row and a full tile"


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_the_expert_kernels_add_the_experts_biases(dt):
    layer = _layer(640, 384, dt, bias=True)
    assert layer.experts[3].proj.linear.bias is not None and layer.experts[3].fc_2.linear.bias.abs().max() > 0
    _check_kernels(layer, _x(16, 640, dt, 12), dt)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_the_expert_kernels_take_a_strided_x(dt):
    """a column slice of a wider tensor: the row stride is not the row length, and the gather reads through it"""
    layer = _layer(256, 128, dt)
    wide = _x(16, 256 + 64, dt, 13)
    x = wide[:, 32:32 + 256]
    assert x.stride(0) == 320 and not x.is_contiguous()
    _check_kernels(layer, x, dt)


# ---- 2. module level -----------------------------------------------------------------------------------------------------------
def _forbid_reads(monkeypatch):
    from fastmax_experiments_amd import moe

    def refuse(offsets):
        raise AssertionError("the device-routed call read its experts' row counts back")
    monkeypatch.setattr(moe, "_read_offsets", refuse)


def _count_reads(monkeypatch):
    from fastmax_experiments_amd import moe
    reads, real = [], moe._read_offsets
    monkeypatch.setattr(moe, "_read_offsets", lambda offsets: reads.append(offsets.numel()) or real(offsets))
    return reads


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("n_embd, inter", [(128, 128), (640, 384)])
def test_the_module_gives_the_same_bits_device_routed_and_not(n_embd, inter, dt, monkeypatch):
    layer = _layer(n_embd, inter, dt)
    want = {}
    with torch.no_grad():
        for M in (1, 2, 16):
            want[M] = layer(_x(M, n_embd, dt, 20 + M).view(1, M, n_embd))
    layer.device_routed = True
    try:
        _forbid_reads(monkeypatch)
        with torch.no_grad():
            for M in (1, 2, 16):
                got = layer(_x(M, n_embd, dt, 20 + M).view(1, M, n_embd))
                assert got.shape == (1, M, n_embd) and torch.equal(got, want[M]), M
        monkeypatch.undo()
        # more rows than a tile, and a call that needs a gradient: the old route, one read each
        reads = _count_reads(monkeypatch)
        with torch.no_grad():
            y17 = layer(_x(17, n_embd, dt, 40))
        assert reads == [layer.n_expert + 1]
        x = _x(2, n_embd, dt, 22).requires_grad_(True)
        y = layer(x)
        assert reads == [layer.n_expert + 1] * 2 and y.requires_grad
        y.sum().backward()
        assert x.grad is not None and torch.equal(y.detach(), want[2].view(2, n_embd))
        layer.device_routed = False
        with torch.no_grad():
            assert torch.equal(layer(_x(17, n_embd, dt, 40)), y17)
    finally:
        layer.device_routed = False


def test_the_table_follows_its_weights():
    """the table is rebuilt when a weight is written or replaced, and not otherwise"""
    layer = _layer(128, 128, "bf16", seed=6)
    first = layer.expert_table()
    assert layer.expert_table() is first
    x = _x(4, 128, "bf16", 30)
    layer.device_routed = True
    try:
        with torch.no_grad():
            before = layer(x)
            lin = layer.experts[0].fc_1.linear
            lin.load_dense(torch.randn(128, 128, generator=torch.Generator().manual_seed(31)).to(torch.bfloat16).cuda() * 0.1)
            for e in range(1, layer.n_expert):                                    # every token now differs wherever it went
                layer.experts[e].fc_1.linear.load_dense(lin.dequantize(torch.bfloat16) * (1.0 + e))
            after = layer(x)
            assert layer.expert_table() is not first and not torch.equal(after, before)
            layer.device_routed = False
            assert torch.equal(layer(x), after)
    finally:
        layer.device_routed = False
        _layer.cache_clear()                                                      # this layer's weights were overwritten


# ---- 3. capture ------------------------------------------------------------------------------------------------------------------
def test_a_recorded_layer_follows_the_routing_of_the_rows_it_is_replayed_on():
    from fastmax_experiments_amd import moe
    layer = _layer(256, 128, "bf16", seed=7)
    k = layer.n_expert_per_token
    a, b = _x(3, 256, "bf16", 50), _x(3, 256, "bf16", 51)
    with torch.no_grad():
        sets = [moe.route(layer.gate(x), k)[0].tolist() for x in (a, b)]
        assert sets[0] != sets[1], "the rows replayed should route to other experts than the rows recorded"
        want_a, want_b = layer(a), layer(b)                                       # the eager route
    layer.device_routed = True
    try:
        x_static = a.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(2):
                layer(x_static)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph), torch.no_grad():
            y_static = layer(x_static)
        graph.replay()
        assert torch.equal(y_static, want_a)
        x_static.copy_(b)
        graph.replay()
        assert torch.equal(y_static, want_b)
    finally:
        layer.device_routed = False


def test_the_table_cannot_be_built_inside_a_capture():
    fresh = _layer(128, 128, "bf16", seed=8)
    assert fresh._table is None
    fresh.device_routed = True
    try:
        x = _x(2, 128, "bf16", 52)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph), torch.no_grad():
            doubled = x + x                                                       # the recording itself is a sound one
            with pytest.raises(RuntimeError, match="while a stream is capturing"):
                fresh.expert_table()
        graph.replay()
        assert fresh._table is None and torch.equal(doubled, x + x)
        with torch.no_grad():
            y = fresh(x)                                                          # outside, the same call builds it
        fresh.device_routed = False
        with torch.no_grad():
            assert torch.equal(fresh(x), y)
    finally:
        fresh.device_routed = False


# ---- 4. generation ---------------------------------------------------------------------------------------------------------------
VOCAB, PROMPT, TOTAL = 97, 5, 11


@functools.lru_cache(maxsize=None)
def _model():
    from fastmax_experiments_amd.attention_block import build_rope_cache
    from fastmax_experiments_amd.block import Block, BlockStack
    from fastmax_experiments_amd.generate import NextTokenHead
    torch.manual_seed(8)
    blocks = [Block(n_embd=128, n_head=4, intermediate_size=128, mlp_class="LLaMAMoE", n_expert=4, n_expert_per_token=2)
              .to(torch.bfloat16).quantize_base() for _ in range(2)]
    stack = BlockStack(blocks).cuda().eval()
    head = NextTokenHead(128, VOCAB).to(torch.bfloat16).cuda().eval()
    wte = torch.randn(VOCAB, 128).to(torch.bfloat16).cuda()
    cos, sin = (t.to(torch.bfloat16) for t in build_rope_cache(TOTAL, stack.blocks[0].attn.rope_n_elem, device="cuda"))
    g = torch.Generator().manual_seed(9)
    prompt = torch.randint(0, VOCAB, (2, PROMPT), generator=g).cuda()
    other = torch.randint(0, VOCAB, (2, 3), generator=g).cuda()
    return dict(stack=stack, head=head, wte=wte, cos=cos, sin=sin, prompt=prompt, other=other)


def _states(B=2):
    from fastmax_experiments_amd.decode import FastmaxDecodeState
    return [FastmaxDecodeState(B, 4, 32, "cuda", p=2, n_query_groups=4) for _ in range(2)]


def _route_all(m, on):
    for blk in m["stack"].blocks:
        blk.mlp.device_routed = on


def _eager(m, prompt, n, seed, **kw):
    from fastmax_experiments_amd.generate import Sampler, generate
    return generate(m["wte"], m["stack"], m["head"], _states(), prompt, n, cos=m["cos"], sin=m["sin"], sampler=Sampler(seed), **kw)


SAMPLING = {"greedy": dict(temperature=0.0), "sampled": dict(temperature=1.0, top_k=20)}


@pytest.mark.parametrize("sampling", list(SAMPLING))
def test_generation_gives_the_same_tokens_device_routed_eager_and_graphed(sampling, monkeypatch):
    from fastmax_experiments_amd import moe
    from fastmax_experiments_amd.generate import GraphedDecoder, Sampler, generate
    m, kw = _model(), SAMPLING[sampling]
    try:
        _route_all(m, False)
        want = _eager(m, m["prompt"], TOTAL, 21, **kw)
        want_other = _eager(m, m["other"], 3 + TOTAL - PROMPT, 22, **kw)
        assert want.shape == (2, TOTAL) and torch.equal(want[:, :PROMPT], m["prompt"])
        _route_all(m, True)
        # the eager loop on the new route, with every routing decision recorded and no row count read back after the prompt
        picked, real = [], moe.route

        def recording(router, k):
            out = real(router, k)
            picked.append(out[0].clone())
            return out
        monkeypatch.setattr(moe, "route", recording)
        _forbid_reads(monkeypatch)                                               # the prompt is 10 rows, the steps 2: all on the new route
        got = _eager(m, m["prompt"], TOTAL, 21, **kw)
        monkeypatch.undo()
        assert torch.equal(got, want)
        steps = TOTAL - PROMPT - 1
        assert len(picked) == 2 * (1 + steps)
        per_layer = [{tuple(map(tuple, e.tolist())) for e in picked[2 + layer::2]} for layer in range(2)]      # the decode steps
        assert max(len(s) for s in per_layer) >= 2, "no layer changed its experts across the steps: the seed shows nothing"
        # one graph replay per token
        states = _states()
        decoder = GraphedDecoder(m["wte"], m["stack"], m["head"], states, cos=m["cos"], sin=m["sin"], max_len=TOTAL, **kw)
        assert decoder.captures == 0 and decoder.replays == 0
        sampler = Sampler(21)
        got = decoder.generate(m["prompt"], TOTAL, sampler)
        assert got.shape == (2, TOTAL) and torch.equal(got, want)
        assert decoder.captures == 1 and decoder.replays == steps and sampler.draws == TOTAL - PROMPT
        assert not decoder.cursor.read()["overflow"]
        # another prompt of another length through the same graph
        for s in states:
            s.reset()
        got = generate(m["wte"], m["stack"], m["head"], states, m["other"], 3 + TOTAL - PROMPT, cos=m["cos"], sin=m["sin"],
                       sampler=Sampler(22), graphed=decoder, **kw)
        assert got.shape == want_other.shape and torch.equal(got, want_other)
        assert decoder.captures == 1 and decoder.replays == 2 * steps
        assert all(s.count == 3 + TOTAL - PROMPT - 1 for s in states)
    finally:
        _route_all(m, False)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_graphed_decoder_still_refuses_what_it_cannot_record():
    from fastmax_experiments_amd.generate import GraphedDecoder
    m = _model()
    kw = dict(cos=m["cos"], sin=m["sin"], max_len=TOTAL)
    try:
        _route_all(m, True)
        m["stack"].blocks[1].mlp.device_routed = False
        with pytest.raises(NotImplementedError, match="row counts"):
            GraphedDecoder(m["wte"], m["stack"], m["head"], _states(), **kw)
        _route_all(m, True)
        with pytest.raises(NotImplementedError, match="at most 16 rows"):
            GraphedDecoder(m["wte"], m["stack"], m["head"], _states(17), **kw)
        assert GraphedDecoder(m["wte"], m["stack"], m["head"], _states(16), **kw).captures == 0
    finally:
        _route_all(m, False)
