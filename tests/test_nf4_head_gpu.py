"""The next-token head on a biased or NF4-quantised lm_head on an MI355X (csrc/last_logits.hip, include/fastmax_hip_head.h,
fastmax_experiments_amd/generate.py).

1. last_logits on NF4 codes against float64.  The weight the reference multiplies is the HOST path of nf4_dequantize on the
   codes and scales moved to the CPU, rounded to the dtype: no device code produces a value the kernel is checked against.  Per
   logit |err| <= (C + 3) 2^-24 sum_c |x_c w^_c|, test_next_token_gpu.py's bound for float32 accumulation of exact products (one
   rounding per add at unit roundoff 2^-24); a 16-bit output adds its own rounding, relative 2^-8 (bf16) or 2^-11 (fp16).  A
   product rounded to bfloat16 on the way (x in float32 or float16 through a bf16 matrix instruction) would miss it by orders of
   magnitude.  Two calls: equal bits.
2. rows of a batch alone, a slice of five, a contiguous copy of x and x off every 16-byte boundary: equal bits.
3. the first 500 of 576 quantised rows against the first 500 columns of all 576: equal bits.
4. the bias: one float32 add behind the sum, on the dense and the NF4 route; a null bias through the new dense entry point
   against fastmax_hip_last_logits: equal bits.
5. a bf16 model (two pythia-14m blocks, n_embd 128, 515 of 576 vocabulary rows) under a head with a bias, quantised plain and
   double-quantised, and the same with NeoX blocks and a LayerNorm: the head against float64 and against its tensor-op
   restatement, greedy and sampled generation, and the graphed loop against the eager one."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
OUT_ROUNDING = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
FORMS = {"plain": False, "double": True}
# (B, C, V).  C = 64: one block per row; 192, 2112: no multiple of 128 and of 512 (lanes with one piece more than others);
# B = 17: three passes over the codes (8 + 8 + 1); V = 1, 33, 63, 257, 515, 4099: no multiple of the 16 rows of a workgroup;
# (17, 2112, 257): 8481 scale blocks, so the double-quantised form spans 34 blocks of 256 and ends inside one
LOGIT_SHAPES = [(1, 128, 515), (3, 64, 63), (2, 64, 1), (9, 192, 33), (17, 2112, 257), (1, 2048, 4099)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from fastmax_experiments_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


# ---- 1. logits -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _codes(C, rows):
    """random rows quantised by the host codec, once for both scale forms: (packed codes, fp32 block scales)"""
    from fastmax_experiments_amd.lora import nf4_quantize
    return nf4_quantize(torch.randn(rows, C, generator=torch.Generator().manual_seed(7 * C + rows)) * 0.05)


@functools.lru_cache(maxsize=None)
def _quantised(C, V, form, rows=None):
    """an NF4Linear of V (or `rows` >= V) random rows on the device, and its host copy"""
    from fastmax_experiments_amd.lora import BLOCK, NF4Linear, Params4bit, absmax_double_quantize
    rows = V if rows is None else rows
    packed, absmax = _codes(C, rows)
    state = [absmax.clone(), torch.Size((rows, C)), torch.float32, BLOCK, None, "nf4"]
    if FORMS[form]:
        q, absmax2, offset, code2 = absmax_double_quantize(absmax)
        state[0], state[4] = q, [offset, [absmax2, code2]]
    lin = NF4Linear(C, rows, bias=False)
    lin.weight = Params4bit(packed.clone(), False, state)
    return copy.deepcopy(lin).cuda(), lin


@functools.lru_cache(maxsize=None)
def _case(B, C, V, dtname, form):
    """x: the last position of a (B, 5, C) tensor, as a view; the device layer; float64 logits and their bound (read-only)"""
    dt = DTYPES[dtname]
    dev, host = _quantised(C, V, form)
    assert host.weight.device.type == "cpu" and all(t.device.type == "cpu" for t in _flat(host.weight.quant_state))
    hidden = torch.randn(B, 5, C, generator=torch.Generator().manual_seed(1000 * C + V + B)).to(dt).cuda()
    x = hidden[:, -1]
    assert x.stride() == (5 * C, 1)
    x64 = x.double().cpu().numpy()
    w64 = host.dequantize(dt).double().numpy()                    # the host path: tensor ops on CPU tensors
    want = x64 @ w64.T
    bound = (C + 3) * 2.0 ** -24 * (np.abs(x64) @ np.abs(w64).T)
    want.setflags(write=False)
    bound.setflags(write=False)
    return x, dev, want, bound


def _flat(state):
    for t in state:
        if isinstance(t, (list, tuple)) and not isinstance(t, torch.Size):
            yield from _flat(t)
        elif isinstance(t, torch.Tensor):
            yield t


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dtname", list(DTYPES))
@pytest.mark.parametrize("B,C,V", LOGIT_SHAPES)
def test_nf4_last_logits_against_float64(B, C, V, dtname, form):
    from fastmax_experiments_amd.generate import last_logits
    dt = DTYPES[dtname]
    x, lin, want, bound = _case(B, C, V, dtname, form)
    assert lin.double_quant == FORMS[form] and lin.weight.quant_state[0].numel() == V * C // 64
    for out_dt in dict.fromkeys((torch.float32, dt)):
        got = last_logits(x, lin, out_dt)
        assert got.shape == (B, V) and got.dtype == out_dt
        err = np.abs(got.double().cpu().numpy() - want)
        limit = bound + OUT_ROUNDING[out_dt] * (np.abs(want) + bound)
        worst = float((err / np.maximum(limit, 1e-300)).max())
        print(f"nf4 last_logits {form} {dtname} -> {out_dt} B={B} C={C} V={V}: worst err / bound {worst:.3f}")
        assert (err <= limit).all()
        assert torch.equal(got, last_logits(x, lin, out_dt)), "two calls differ"
        assert torch.equal(got, last_logits(x, lin.weight, out_dt)), "the Params4bit alone differs from its layer"


def test_the_device_dequantiser_returns_the_weight_the_head_scores():
    """the reference above is the host codec's; the other NF4 kernels multiply nf4_dequantize's device output: the same bits"""
    for form in FORMS:
        dev, host = _quantised(2112, 257, form)
        for dt in (torch.float32, torch.bfloat16):
            assert torch.equal(dev.dequantize(dt).cpu(), host.dequantize(dt)), (form, dt)


# ---- 2. batch, stride and load route ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dtname", list(DTYPES))
def test_a_rows_nf4_logits_do_not_depend_on_its_batch_or_stride(dtname, form):
    from fastmax_experiments_amd.generate import last_logits
    x, lin, _, _ = _case(17, 2112, 257, dtname, form)
    batch = last_logits(x, lin)
    for b in range(17):
        assert torch.equal(batch[b:b + 1], last_logits(x[b:b + 1], lin)), f"row {b} alone differs from row {b} of the batch"
    assert torch.equal(batch[3:8], last_logits(x[3:8], lin))
    dense = x.contiguous()
    assert dense.stride() == (2112, 1) and torch.equal(batch, last_logits(dense, lin))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dtname", list(DTYPES))
@pytest.mark.parametrize("B,C,V", [(3, 2112, 257), (9, 192, 33)])
def test_x_off_the_sixteen_byte_boundaries_gives_equal_bits(B, C, V, dtname, form):
    from fastmax_experiments_amd.generate import last_logits
    dt = DTYPES[dtname]
    lin, _ = _quantised(C, V, form)
    x = torch.randn(B, C, generator=torch.Generator().manual_seed(B + C)).to(dt).cuda()
    wide = torch.zeros(B, C + 3, dtype=dt, device="cuda")
    off = wide[:, 1:C + 1]                                        # one element past a boundary, an odd row stride
    off.copy_(x)
    assert x.data_ptr() % 16 == 0 and off.data_ptr() % 16 != 0 and off.stride() == (C + 3, 1)
    for out_dt in dict.fromkeys((torch.float32, dt)):
        assert torch.equal(last_logits(x, lin, out_dt), last_logits(off, lin, out_dt))


# ---- 3. vocab_size < padded_vocab_size -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dtname", list(DTYPES))
def test_scoring_the_first_rows_of_a_padded_weight(dtname, form):
    from fastmax_experiments_amd.generate import last_logits
    lin, _ = _quantised(128, 500, form, rows=576)
    assert tuple(lin.weight.quant_state[1]) == (576, 128)
    x = torch.randn(3, 128, generator=torch.Generator().manual_seed(12)).to(DTYPES[dtname]).cuda()
    every = last_logits(x, lin)
    first = last_logits(x, lin, rows=500)
    assert every.shape == (3, 576) and first.shape == (3, 500) and torch.equal(first, every[:, :500])


# ---- 4. the bias -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtname", list(DTYPES))
@pytest.mark.parametrize("route", ["dense", "plain", "double"])
def test_the_bias_is_one_float32_add_behind_the_sum(route, dtname):
    from fastmax_experiments_amd.generate import last_logits
    dt = DTYPES[dtname]
    B, C, V = 9, 192, 259
    g = torch.Generator().manual_seed(31)
    x = torch.randn(B, 5, C, generator=g).to(dt).cuda()[:, -1]
    bias = torch.randn(V + 5, generator=g).to(dt).cuda()
    weight = torch.randn(V, C, generator=g).to(dt).cuda() if route == "dense" else _quantised(C, V, route)[0]
    bare = last_logits(x, weight)
    assert bare.dtype == torch.float32
    got = last_logits(x, weight, bias=bias[:V])
    assert torch.equal(got, bare + bias[:V].float())
    assert not torch.equal(got, bare)
    assert torch.equal(last_logits(x, weight, bias=bias, rows=V - 3), got[:, :V - 3])          # a longer bias, fewer rows
    if dt != torch.float32:                                       # a 16-bit output: the float32 sum with its bias, rounded once
        assert torch.equal(last_logits(x, weight, dt, bias=bias[:V]), got.to(dt))


@pytest.mark.parametrize("dtname", list(DTYPES))
@pytest.mark.parametrize("B,C,V,col0", [(17, 2056, 257, 8), (3, 100, 63, 8), (9, 96, 63, 1), (1, 2048, 4099, 8)])
def test_a_null_bias_gives_the_bits_of_the_entry_point_without_one(B, C, V, col0, dtname):
    """fastmax_hip_last_logits_bias with bias = NULL against fastmax_hip_last_logits: 16-byte pieces, a short last piece
    (C = 100) and the element route (columns from 1), in one, two and three passes"""
    from fastmax_experiments_amd import ops
    from fastmax_experiments_amd.generate import last_logits
    dt = DTYPES[dtname]
    g = torch.Generator().manual_seed(1000 * C + V + B)
    x = torch.randn(B, 5, C, generator=g).to(dt).cuda()[:, -1]
    w = torch.randn(V + 2, C + 16, generator=g).to(dt).cuda()[1:V + 1, col0:col0 + C]
    for out_dt in dict.fromkeys((torch.float32, dt)):
        want = last_logits(x, w, out_dt)
        got = torch.empty_like(want)
        ops._call("fastmax_hip_last_logits_bias", x.device,
                  (x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), None, got.data_ptr(), got.stride(0), B, V, C, ops._DT[dt], ops._DT[out_dt]))
        assert torch.equal(got, want)


# ---- 5. the head and generation --------------------------------------------------------------------------------------------------
PADDED, VOCAB, PROMPT, NEW = 576, 515, 5, 8
MODELS = ["block-plain", "block-double", "neox-double"]


@functools.lru_cache(maxsize=None)
def _model(name):
    from fastmax_experiments_amd.attention_block import build_rope_cache
    from fastmax_experiments_amd.block import Block, BlockStack
    from fastmax_experiments_amd.generate import NextTokenHead
    from fastmax_experiments_amd.neox_block import NeoXBlock, NeoXStack
    kind, form = name.split("-")
    dt = torch.bfloat16
    torch.manual_seed(3)
    if kind == "neox":
        stack = NeoXStack([NeoXBlock.from_config("pythia-14m", attn_alg="fastmax") for _ in range(2)]).to("cuda", dt).eval()
        head = NextTokenHead(128, PADDED, VOCAB, norm_class="LayerNorm", lm_head_bias=True)
        torch.nn.init.normal_(head.ln_f.bias, std=0.2)
    else:
        stack = BlockStack([Block.from_config("pythia-14m", attn_alg="fastmax") for _ in range(2)]).to("cuda", dt).eval()
        head = NextTokenHead(128, PADDED, VOCAB, lm_head_bias=True)
    torch.nn.init.normal_(head.ln_f.weight, mean=1.0, std=0.2)
    torch.nn.init.normal_(head.lm_head.bias, std=0.5)
    head = head.to("cuda", dt).eval().quantize_base(FORMS[form])
    wte = torch.randn(PADDED, 128).to(dt).cuda()
    cos, sin = build_rope_cache(PROMPT + NEW, stack.blocks[0].attn.rope_n_elem, device="cuda")
    g = torch.Generator().manual_seed(4)
    prompt = torch.randint(0, VOCAB, (2, PROMPT), generator=g).cuda()
    other = torch.randint(0, VOCAB, (2, 3), generator=g).cuda()
    return dict(name=name, stack=stack, head=head, wte=wte, cos=cos, sin=sin, prompt=prompt, other=other)


def _states(B=2):
    from fastmax_experiments_amd.decode import FastmaxDecodeState
    return [FastmaxDecodeState(B, 4, 32, "cuda", p=2, n_query_groups=4) for _ in range(2)]


def _generate(m, states=None, prompt=None, n=PROMPT + NEW, **kw):
    from fastmax_experiments_amd.generate import generate
    prompt = m["prompt"] if prompt is None else prompt
    return generate(m["wte"], m["stack"], m["head"], _states() if states is None else states, prompt, n, cos=m["cos"], sin=m["sin"],
                    **kw)


def _normed(head, last):
    """the rows the fused route's head product reads: the norm kernel on the last position"""
    from fastmax_experiments_amd.block import rms_norm_forward
    from fastmax_experiments_amd.neox_block import LayerNorm, layer_norm_forward
    if isinstance(head.ln_f, LayerNorm):
        return layer_norm_forward(last, head.ln_f.weight.detach(), head.ln_f.bias.detach(), head.ln_f.eps)[1]
    return rms_norm_forward(last, None, head.ln_f.weight.detach(), head.ln_f.eps, head.ln_f.add_unit_offset)[1]


@pytest.mark.parametrize("name", MODELS)
def test_head_logits_against_float64_and_the_tensor_op_restatement(name):
    """Each route against float64 on ITS OWN normalised rows (the norm kernel's / the norm's tensor ops'; they may differ in a last
    bf16 digit).  Fused: the bound of part 1 plus the bias add's rounding, 2^-24 of the result.  Restated: F.linear in bf16 -- a
    float32 accumulation under the same bound, then up to two roundings to bf16 (the product, the sum with the bias) and the
    bias itself rounded to bf16 (the layer keeps it in float32; the model here was cast to bf16 first, so that is exact).  The
    two against each other: the sum of both limits plus what the difference of the normalised rows is worth."""
    m = _model(name)
    head = m["head"]
    from fastmax_experiments_amd.lora import NF4Linear
    assert isinstance(head.lm_head, NF4Linear) and head.lm_head.bias is not None and head.lm_head.bias.dtype == torch.float32
    x = torch.randn(3, 4, 128, generator=torch.Generator().manual_seed(8)).to(torch.bfloat16).cuda()
    w64 = copy.deepcopy(head.lm_head).cpu().dequantize(torch.bfloat16).double().numpy()[:VOCAB]
    b64 = head.lm_head.bias.detach().double().cpu().numpy()[:VOCAB]
    assert torch.equal(head.lm_head.bias.to(torch.bfloat16).float(), head.lm_head.bias)

    def reference(n):
        n64 = n.double().cpu().numpy()
        want = n64 @ w64.T + b64
        return n64, want, (128 + 3) * 2.0 ** -24 * (np.abs(n64) @ np.abs(w64).T)

    with torch.no_grad():
        fused = head.logits(x)
        n_k = _normed(head, x[:, -1])
        head.fused = False
        try:
            restated = head.logits(x)
            n_e = head.ln_f._eager(x)[:, -1]
        finally:
            head.fused = True
    assert fused.shape == restated.shape == (3, VOCAB) and fused.dtype == restated.dtype == torch.float32
    nk64, want_k, bound_k = reference(n_k)
    ne64, want_e, bound_e = reference(n_e)
    limit_k = bound_k + 2.0 ** -24 * (np.abs(want_k) + bound_k)
    limit_e = bound_e + 2 * 2.0 ** -8 * (np.abs(want_e) + np.abs(b64) + bound_e)
    err_k = np.abs(fused.double().cpu().numpy() - want_k)
    err_e = np.abs(restated.double().cpu().numpy() - want_e)
    apart = np.abs(fused.double().cpu().numpy() - restated.double().cpu().numpy())
    moved = np.abs(nk64 - ne64) @ np.abs(w64).T
    print(f"head {name}: fused err / bound {float((err_k / limit_k).max()):.3f}, restated {float((err_e / limit_e).max()):.3f}, "
          f"apart / limit {float((apart / (limit_k + limit_e + moved)).max()):.3f}, "
          f"{int((nk64 != ne64).sum())} of {nk64.size} normalised elements differ")
    assert (err_k <= limit_k).all()
    assert (err_e <= limit_e).all()
    assert (apart <= limit_k + limit_e + moved).all()


@pytest.mark.parametrize("name", MODELS)
def test_greedy_generate_is_the_argmax_of_its_own_nf4_logits(name):
    m = _model(name)
    out = _generate(m, temperature=0.0)
    assert out.shape == (2, PROMPT + NEW) and out.dtype == torch.int64 and torch.equal(out[:, :PROMPT], m["prompt"])
    assert int(out.min()) >= 0 and int(out.max()) < VOCAB
    states = _states()
    pos = torch.arange(PROMPT + NEW, device="cuda")
    with torch.no_grad():
        for a, b in [(0, PROMPT)] + [(t, t + 1) for t in range(PROMPT, PROMPT + NEW - 1)]:
            x = torch.nn.functional.embedding(out[:, a:b], m["wte"])
            h = m["stack"](x, m["cos"][a:b], m["sin"][a:b], pos[a:b], states)
            logits = m["head"].logits(h)
            assert logits.shape == (2, VOCAB) and logits.dtype == torch.float32
            first_max = logits.cpu().numpy().argmax(-1)                         # numpy: the first of equal maxima
            assert np.array_equal(first_max, out[:, b].cpu().numpy()), f"position {b}"


@pytest.mark.parametrize("name", MODELS)
def test_sampled_generate_on_an_nf4_head_reproduces_under_its_seed(name):
    from fastmax_experiments_amd.generate import Sampler
    m = _model(name)
    a = _generate(m, temperature=1.0, top_k=100, sampler=Sampler(21))
    b = _generate(m, temperature=1.0, top_k=100, sampler=Sampler(21))
    c = _generate(m, temperature=1.0, top_k=100, sampler=Sampler(22))
    assert a.shape == (2, PROMPT + NEW) and torch.equal(a, b) and not torch.equal(a, c)
    assert int(a.max()) < VOCAB
    s = Sampler(21)
    _generate(m, temperature=1.0, top_p=0.9, sampler=s)
    assert s.draws == NEW


@pytest.mark.parametrize("sampling", ["greedy", "sampled"])
@pytest.mark.parametrize("name", MODELS)
def test_graphed_generate_on_an_nf4_head_equals_the_eager_loop(name, sampling):
    from fastmax_experiments_amd.generate import GraphedDecoder, Sampler
    m = _model(name)
    kw = dict(temperature=0.0) if sampling == "greedy" else dict(temperature=1.0, top_k=100)
    eager_states, states = _states(), _states()
    decoder = GraphedDecoder(m["wte"], m["stack"], m["head"], states, cos=m["cos"], sin=m["sin"], max_len=PROMPT + NEW, **kw)
    assert decoder.captures == 0 and decoder.replays == 0
    s_eager, s_graph = Sampler(21), Sampler(21)
    want = _generate(m, eager_states, sampler=s_eager, **kw)
    got = decoder.generate(m["prompt"], PROMPT + NEW, s_graph)
    assert got.shape == (2, PROMPT + NEW) and torch.equal(got, want)
    assert s_graph.draws == s_eager.draws == NEW
    for a, b in zip(states, eager_states):
        assert a.count == b.count == PROMPT + NEW - 1 and torch.equal(a.state, b.state)
    assert decoder.captures == 1 and decoder.replays == NEW - 1
    assert not decoder.cursor.read()["overflow"]
    # the same graph on a prompt of another length, under another seed and a draw count that does not start at 0
    for s in states + eager_states:
        s.reset()
    s_eager, s_graph = Sampler(22), Sampler(22)
    s_eager.draws = s_graph.draws = 5
    want = _generate(m, eager_states, m["other"], 3 + NEW, sampler=s_eager, **kw)
    got = _generate(m, states, m["other"], 3 + NEW, sampler=s_graph, graphed=decoder, **kw)
    assert got.shape == (2, 3 + NEW) and torch.equal(got, want)
    assert s_graph.draws == s_eager.draws == 5 + NEW
    for a, b in zip(states, eager_states):
        assert a.count == b.count and torch.equal(a.state, b.state)
    assert decoder.captures == 1 and decoder.replays == 2 * (NEW - 1)


def test_the_scales_cannot_be_first_built_while_a_stream_is_capturing():
    """what GraphedDecoder's eager steps spare the recording: a layer that has never scored refuses to start inside one"""
    from fastmax_experiments_amd.generate import last_logits
    from fastmax_experiments_amd.lora import NF4Linear, scales_cached
    lin = NF4Linear(64, 16, bias=False)
    lin.load_dense(torch.randn(16, 64, generator=torch.Generator().manual_seed(2)), double_quant=True)
    lin = lin.cuda()
    x = torch.randn(2, 64, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        doubled = x + x                                                           # the recording itself is a sound one
        with pytest.raises(RuntimeError, match="while a stream is capturing"):
            last_logits(x, lin)
    graph.replay()
    assert not scales_cached(lin) and torch.equal(doubled, x + x)
    want = last_logits(x, lin)                                                    # outside, the same call builds them
    assert scales_cached(lin)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = last_logits(x, lin)                                                 # and a recording may then use them
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, want)
