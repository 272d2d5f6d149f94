"""The decode cursor on an MI355X (csrc/decode_cursor.hip, generate.DecodeCursor / GraphedDecoder).  Everything here is a copy, a
seeded draw or a loop of kernels that the eager loop runs too, so every comparison is for equal bits.

1. feed: the embedding rows against F.embedding and the rope rows against cos[pos:pos + 1], on the 16-byte route and on the element
   route, inside canary-filled buffers; the cursor moves by exactly one per feed + sample pair; the guards.
2. sample: eight consecutive cursor draws against Sampler(seed).sample at the same draw numbers, from draw 0 and from 2^32 - 2
   (the low word carries into the high one); out, tok and done against the tokens.
3. GraphedDecoder.generate against generate(): tokens, sampler.draws, every state cache, one capture, one replay per token after
   the first, a second prompt of another length under another seed on the same graph.
4. eos: the trimmed output against generate(eos_id=...) at poll 1 and 3.
5. refusals."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CANARY = 7.0
ROWS, ROPE_ROWS, ROPE_COLS, N_COLS = 37, 13, 16, 8          # embedding rows; the rope cache is (13, 16), 8 columns are fed


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from fastmax_experiments_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


# ---- 1. feed -----------------------------------------------------------------------------------------------------------------------
def _feed_operands(C, dt, aligned):
    """wte (ROWS, C) and cos, sin (ROPE_ROWS, ROPE_COLS): whole tensors (rows on 16-byte boundaries where C allows), or views of
    wider ones from column 1, which no 16-byte piece fits"""
    g = torch.Generator().manual_seed(100 * C + aligned)
    off = 0 if aligned else 1
    wide = torch.randn(ROWS + 2, C + 8, generator=g).to(dt).cuda()
    rope = [torch.randn(ROPE_ROWS, ROPE_COLS + 8, generator=g).to(dt).cuda() for _ in range(2)]
    wte = wide[1:ROWS + 1, off:off + C]
    cos, sin = (t[:, off:off + ROPE_COLS] for t in rope)
    return wte, cos, sin


def _canaries(B, C, dt):
    x = torch.full((B + 2, C), CANARY, dtype=dt, device="cuda")
    rows = torch.full((2, 3, N_COLS), CANARY, dtype=dt, device="cuda")
    return x, rows


def _untouched(t):
    return bool((t == CANARY).all())


@pytest.mark.parametrize("dtname", list(DTYPES))
@pytest.mark.parametrize("C,aligned", [(128, True), (100, False), (100, True)], ids=["C128-pieces", "C100-elements", "C100-whole"])
def test_feed_copies_the_embedding_and_the_rope_rows(C, aligned, dtname):
    from fastmax_experiments_amd.generate import DecodeCursor
    dt = DTYPES[dtname]
    wte, cos, sin = _feed_operands(C, dt, aligned)
    es = wte.element_size()
    # the 16-byte route needs whole pieces in a row, in both row strides and in both addresses: C = 100 leaves it to float32
    pieces = all(n % 16 == 0 for n in (C * es, wte.stride(0) * es, wte.data_ptr(), cos.data_ptr(), cos.stride(0) * es))
    assert pieces == (aligned and (C == 128 or dt == torch.float32))
    cursor = DecodeCursor("cuda")
    for B in (1, 3):
        for pos in (0, ROPE_ROWS // 2, ROPE_ROWS - 1):
            tok = torch.randint(0, ROWS, (B,), generator=torch.Generator().manual_seed(pos + B)).cuda()
            tok[-1] = ROWS - 1 if pos else 0                                # the table's two ends
            x, rows = _canaries(B, C, dt)
            cursor.arm(pos, 0, 5)
            cursor.feed(tok, wte, x[1:B + 1], cos, sin, rows[0, 1:2], rows[1, 1:2])
            assert torch.equal(x[1:B + 1], torch.nn.functional.embedding(tok, wte)), (B, pos, pieces)
            assert torch.equal(rows[0, 1:2], cos[pos:pos + 1, :N_COLS]) and torch.equal(rows[1, 1:2], sin[pos:pos + 1, :N_COLS])
            assert _untouched(x[0]) and _untouched(x[B + 1]) and _untouched(rows[:, 0]) and _untouched(rows[:, 2])
            assert cursor.read() == dict(pos=pos, next=pos + 1, overflow=False)


@pytest.mark.parametrize("dtname", list(DTYPES))
def test_the_two_routes_of_the_feed_give_equal_bits(dtname):
    from fastmax_experiments_amd.generate import DecodeCursor
    dt = DTYPES[dtname]
    wte, cos, sin = _feed_operands(128, dt, True)
    wte_off, cos_off, sin_off = _feed_operands(128, dt, False)
    for dst, src in ((wte_off, wte), (cos_off, cos), (sin_off, sin)):
        dst.copy_(src)
        assert dst.data_ptr() % 16 != 0 and src.data_ptr() % 16 == 0
    tok = torch.tensor([36, 0, 17], device="cuda")
    got = []
    for w, c, s in ((wte, cos, sin), (wte_off, cos_off, sin_off)):
        x, rows = _canaries(3, 128, dt)
        cursor = DecodeCursor("cuda")
        cursor.arm(6, 0, 5)
        cursor.feed(tok, w, x[1:4], c, s, rows[0, 1:2], rows[1, 1:2])
        got.append((x, rows))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])


def _pair(cursor, logits, tok, out, done=None, eos_id=None, temperature=0.0, top_k=None):
    """one feed + sample pair; the feed moves a row of a tiny table, so that only the cursor matters"""
    B = logits.shape[0]
    wte, rope = torch.zeros(4, 8, device="cuda"), torch.zeros(out.shape[1], 8, device="cuda")
    x, row = torch.zeros(B, 8, device="cuda"), torch.zeros(2, 1, 8, device="cuda")
    cursor.feed(torch.zeros(B, dtype=torch.int64, device="cuda"), wte, x, rope, rope, row[0], row[1])
    cursor.sample(logits, tok, out, done, eos_id, temperature, top_k)


def test_the_cursor_moves_by_exactly_one_per_feed_and_sample_pair():
    from fastmax_experiments_amd.generate import DecodeCursor
    cursor = DecodeCursor("cuda")
    logits = torch.randn(3, 7, generator=torch.Generator().manual_seed(0)).cuda()
    tok = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    out = torch.full((3, 6), -1, dtype=torch.int64, device="cuda")
    cursor.arm(2, 0, 5)
    for pos in (2, 3, 4):
        _pair(cursor, logits, tok, out)
        assert cursor.read() == dict(pos=pos + 1, next=pos + 1, overflow=False)
        assert torch.equal(out[:, pos + 1], logits.argmax(1)) and torch.equal(tok, logits.argmax(1))
    assert bool((out[:, :3] == -1).all())


def test_a_feed_past_the_rope_cache_writes_nothing_and_the_pair_is_a_no_op():
    from fastmax_experiments_amd.generate import DecodeCursor
    dt = torch.bfloat16
    wte, cos, sin = _feed_operands(128, dt, True)
    cursor = DecodeCursor("cuda")
    x, rows = _canaries(3, 128, dt)
    tok = torch.tensor([1, 2, 3], device="cuda")
    cursor.arm(ROPE_ROWS, 0, 5)
    cursor.feed(tok, wte, x[1:4], cos, sin, rows[0, 1:2], rows[1, 1:2])
    assert _untouched(x) and _untouched(rows)
    assert cursor.read() == dict(pos=ROPE_ROWS, next=-1, overflow=True)
    # the sample of that step: nothing is written, the cursor stays; so does a replay too many at the end of out
    logits = torch.randn(3, 7, generator=torch.Generator().manual_seed(0)).cuda()
    sampled = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    out = torch.full((3, ROPE_ROWS + 4), -1, dtype=torch.int64, device="cuda")
    done = torch.zeros(3, dtype=torch.uint8, device="cuda")
    cursor.sample(logits, sampled, out, done, int(logits[0].argmax()))
    assert bool((sampled == -1).all()) and bool((out == -1).all()) and not bool(done.any())
    assert cursor.read() == dict(pos=ROPE_ROWS, next=-1, overflow=True)
    short = torch.full((3, 4), -1, dtype=torch.int64, device="cuda")          # L = 4: column next = 4 does not exist
    cursor.arm(3, 0, 5)
    assert not cursor.read()["overflow"]
    _pair(cursor, logits, sampled, short)
    assert bool((sampled == -1).all()) and bool((short == -1).all())
    assert cursor.read() == dict(pos=3, next=4, overflow=True)


@pytest.mark.parametrize("bad", [ROWS, -1, 2 ** 40])
def test_a_token_outside_the_table_yields_a_zero_row_and_sets_the_flag(bad):
    from fastmax_experiments_amd.generate import DecodeCursor
    for C, aligned in ((128, True), (100, False)):
        wte, cos, sin = _feed_operands(C, torch.float16, aligned)
        cursor = DecodeCursor("cuda")
        x, rows = _canaries(3, C, torch.float16)
        tok = torch.tensor([5, bad, 36], device="cuda")
        cursor.arm(1, 0, 5)
        cursor.feed(tok, wte, x[1:4], cos, sin, rows[0, 1:2], rows[1, 1:2])
        assert torch.equal(x[1], wte[5]) and torch.equal(x[3], wte[36]) and bool((x[2] == 0).all())
        assert _untouched(x[0]) and _untouched(x[4]) and torch.equal(rows[0, 1:2], cos[1:2, :N_COLS])
        assert cursor.read() == dict(pos=1, next=2, overflow=True)


# ---- 2. sample ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_draw", [0, 2 ** 32 - 2], ids=["from0", "carry"])
@pytest.mark.parametrize("V,k,temperature", [(515, 50, 0.8), (7, 3, 0.5), (515, 50, 0.0)])
def test_cursor_draws_equal_the_samplers_at_the_same_draw_numbers(V, k, temperature, first_draw):
    from fastmax_experiments_amd.generate import DecodeCursor, Sampler
    B, seed, draws, pos0 = 64, 2 ** 40 + 9, 8, 3
    logits = torch.from_numpy(np.random.default_rng(V).normal(0, 3, (B, V)).astype(np.float32)).cuda()
    s = Sampler(seed)
    s.draws = first_draw
    want = torch.stack([s.sample(logits, temperature, k) for _ in range(draws)], dim=1)          # (B, draws)
    assert s.draws == first_draw + draws
    if temperature > 0:
        assert not torch.equal(want[:, 0], want[:, 1]) and not torch.equal(want[:, 1], want[:, 2])          # the draws do differ
    eos = int(want[0, 0])
    cursor = DecodeCursor("cuda")
    cursor.arm(pos0, first_draw, seed)
    tok = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    out = torch.full((B, pos0 + 1 + draws), -1, dtype=torch.int64, device="cuda")
    done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    for d in range(draws):
        _pair(cursor, logits, tok, out, done, eos, temperature, k)
        assert torch.equal(tok, want[:, d]), f"draw {first_draw + d}"
        assert torch.equal(done.bool(), (want[:, :d + 1] == eos).any(dim=1))
    assert torch.equal(out[:, pos0 + 1:], want) and bool((out[:, :pos0 + 1] == -1).all())
    assert bool(done[0]) and cursor.read() == dict(pos=pos0 + draws, next=pos0 + draws, overflow=False)


# ---- 3. the whole loop ---------------------------------------------------------------------------------------------------------------
VOCAB, PROMPT, NEW = 515, 5, 8          # test_next_token_gpu.py's model
MODELS = ["fastmax", "linearmax", "fastmax-fused-step", "neox"]


@functools.lru_cache(maxsize=None)
def _model(name):
    from fastmax_experiments_amd.attention_block import build_rope_cache
    from fastmax_experiments_amd.block import Block, BlockStack
    from fastmax_experiments_amd.generate import NextTokenHead
    from fastmax_experiments_amd.neox_block import NeoXBlock, NeoXStack
    alg = "linearmax" if name == "linearmax" else "fastmax"
    torch.manual_seed(3)
    if name == "neox":
        stack = NeoXStack([NeoXBlock.from_config("pythia-14m", attn_alg=alg) for _ in range(2)]).cuda().eval()
        head = NextTokenHead(128, VOCAB, norm_class="LayerNorm").cuda().eval()
    else:
        stack = BlockStack([Block.from_config("pythia-14m", attn_alg=alg) for _ in range(2)]).cuda().eval()
        head = NextTokenHead(128, VOCAB).cuda().eval()
    wte = torch.randn(VOCAB, 128).cuda()
    cos, sin = build_rope_cache(PROMPT + NEW, stack.blocks[0].attn.rope_n_elem, device="cuda")
    g = torch.Generator().manual_seed(4)
    prompt = torch.randint(0, VOCAB, (2, PROMPT), generator=g).cuda()
    other = torch.randint(0, VOCAB, (2, 3), generator=g).cuda()
    return dict(name=name, alg=alg, stack=stack, head=head, wte=wte, cos=cos, sin=sin, prompt=prompt, other=other)


def _states(m, B=2):
    from fastmax_experiments_amd.decode import FastmaxDecodeState, LinearmaxDecodeState
    if m["alg"] == "linearmax":
        return [LinearmaxDecodeState(B, 4, 32, "cuda", n_query_groups=4) for _ in range(2)]
    states = [FastmaxDecodeState(B, 4, 32, "cuda", p=2, n_query_groups=4) for _ in range(2)]
    for s in states:
        s.fused_step = m["name"] == "fastmax-fused-step"
    return states


def _eager(m, states, prompt, n, **kw):
    from fastmax_experiments_amd.generate import generate
    return generate(m["wte"], m["stack"], m["head"], states, prompt, n, cos=m["cos"], sin=m["sin"], **kw)


def _decoder(m, states, **kw):
    from fastmax_experiments_amd.generate import GraphedDecoder
    return GraphedDecoder(m["wte"], m["stack"], m["head"], states, cos=m["cos"], sin=m["sin"], max_len=PROMPT + NEW, **kw)


@pytest.mark.parametrize("sampling", ["greedy", "sampled"])
@pytest.mark.parametrize("name", MODELS)
def test_graphed_generate_equals_the_eager_loop(name, sampling):
    from fastmax_experiments_amd.generate import Sampler, generate
    m = _model(name)
    kw = dict(temperature=0.0) if sampling == "greedy" else dict(temperature=1.0, top_k=100)
    eager_states, states = _states(m), _states(m)
    decoder = _decoder(m, states, **kw)
    assert decoder.captures == 0 and decoder.replays == 0
    s_eager, s_graph = Sampler(21), Sampler(21)
    want = _eager(m, eager_states, m["prompt"], PROMPT + NEW, sampler=s_eager, **kw)
    got = decoder.generate(m["prompt"], PROMPT + NEW, s_graph)
    assert got.shape == (2, PROMPT + NEW) and torch.equal(got, want)
    assert s_graph.draws == s_eager.draws == NEW
    for a, b in zip(states, eager_states):
        assert a.count == b.count == PROMPT + NEW - 1 and torch.equal(a.state, b.state)
    assert decoder.captures == 1 and decoder.replays == NEW - 1
    assert not decoder.cursor.read()["overflow"]
    # the same graph on a prompt of another length, under another seed and a draw count that does not start at 0, through generate()
    for s in states + eager_states:
        s.reset()
    s_eager, s_graph = Sampler(22), Sampler(22)
    s_eager.draws = s_graph.draws = 5
    want = _eager(m, eager_states, m["other"], 3 + NEW, sampler=s_eager, **kw)
    got = generate(m["wte"], m["stack"], m["head"], states, m["other"], 3 + NEW, cos=m["cos"], sin=m["sin"], sampler=s_graph,
                   graphed=decoder, **kw)
    assert got.shape == (2, 3 + NEW) and torch.equal(got, want)
    assert s_graph.draws == s_eager.draws == 5 + NEW
    for a, b in zip(states, eager_states):
        assert a.count == b.count and torch.equal(a.state, b.state)
    assert decoder.captures == 1 and decoder.replays == 2 * (NEW - 1)
    with pytest.raises(ValueError, match="graphed was built from other"):
        generate(m["wte"], m["stack"], m["head"], states, m["other"], 3 + NEW, cos=m["cos"], sin=m["sin"], graphed=decoder,
                 **dict(kw, temperature=0.5))


# ---- 4. eos --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ["two_prompts", "one_prompt_twice"])
@pytest.mark.parametrize("name", ["fastmax", "linearmax"])
def test_graphed_generate_stops_where_the_eager_loop_stops(name, rows):
    """test_generate_stops_once_every_row_has_produced_eos's two settings: eos_id = the first generated token of row 0"""
    m = _model(name)
    prompt = m["prompt"] if rows == "two_prompts" else m["prompt"][:1].expand(2, PROMPT).contiguous()
    full = _eager(m, _states(m), prompt, PROMPT + NEW, temperature=0.0)
    eos = int(full[0, PROMPT])
    want = _eager(m, _states(m), prompt, PROMPT + NEW, temperature=0.0, eos_id=eos)
    if rows == "one_prompt_twice":
        assert want.shape == (2, PROMPT + 1)
    states = _states(m)
    decoder = _decoder(m, states, temperature=0.0, eos_id=eos)
    assert decoder.poll == 16
    for poll in (1, 3):
        for s in states:
            s.reset()
        decoder.poll = poll
        before = decoder.replays
        got = decoder.generate(prompt, PROMPT + NEW)
        assert got.shape == want.shape and torch.equal(got, want), f"poll {poll}"
        n = want.shape[1]
        ran = decoder.replays - before
        assert n - PROMPT - 1 <= ran <= min(NEW - 1, -(-(n - PROMPT - 1) // poll) * poll), f"poll {poll}: {ran} replays for {n} tokens"
        assert all(s.count == n - 1 for s in states)
    assert decoder.captures == 1


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def test_what_a_recorded_graph_would_freeze_is_refused_before_any_capture():
    from fastmax_experiments_amd.decode import FastmaxDecodeState
    m = _model("fastmax")
    first_order = [FastmaxDecodeState(2, 4, 32, "cuda", p=1) for _ in range(2)]
    with pytest.raises(NotImplementedError, match="by value"):
        _decoder(m, first_order)
    m["head"].fused = False
    try:
        with pytest.raises(ValueError, match="torch's generator"):
            _decoder(m, _states(m))
        m["head"].fused = True
        decoder = _decoder(m, _states(m))
        m["head"].fused = False
        with pytest.raises(ValueError, match="torch's generator"):
            decoder.generate(m["prompt"], PROMPT + NEW)
        assert decoder.captures == 0 and decoder.replays == 0
    finally:
        m["head"].fused = True
