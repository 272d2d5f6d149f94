"""The next-token head on an MI355X (csrc/last_logits.hip, csrc/next_token.hip, fastmax_experiments_amd/generate.py) against
float64 and the numpy restatement (next_token_ref.py).

1. last_logits against float64, per logit |err| <= (C + 3) 2^-24 sum_c |x_c w_c|: one rounding per product and per add at
   unit roundoff 2^-24 (the fused multiply-adds round less often).  A 16-bit output adds its own rounding, relative 2^-8 (bf16)
   or 2^-11 (fp16) of the float32 value.  Rows of a batch against the same rows alone, two calls, and the 16-byte route
   against the element route: equal bits.  The bits themselves against tests/golden/last_logits_*.npz.
2. the keep mask element for element against the restatement: designed ties and random rows.
3. temperature 0 against argmax.
4. sampled tokens against the restatement wherever the float64 gap between the two best scores is >= 1e-3: scores stay below
   512 in magnitude, where a float32 ulp is 6e-5, and each carries under 1e-4 of rounding error (the division, the two
   logarithms, the add).  Closer cases are left out; at most 1 % may be.
5. generate through two pythia-14m blocks on both decode state caches."""
import numpy as np
import pytest
import torch

import next_token_ref as ref
from conftest import load_golden
from test_next_token_cpu import tie_cases

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
OUT_ROUNDING = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
LOGIT_SHAPES = [(1, 128, 515), (3, 100, 63), (17, 2056, 257), (2, 64, 1), (1, 2048, 4099)]          # (B, C, V)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from fastmax_experiments_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


# ---- 1. logits -------------------------------------------------------------------------------------------------------------------
def _logit_operands(B, C, V, dt, col0=8):
    """x: the last position of a (B, 5, C) tensor, as a view; W: rows 1 .. V and columns col0 .. col0 + C of a wider matrix"""
    g = torch.Generator().manual_seed(1000 * C + V + B)
    hidden = torch.randn(B, 5, C, generator=g).to(dt).cuda()
    wide = torch.randn(V + 2, C + 16, generator=g).to(dt).cuda()
    x, w = hidden[:, -1], wide[1:V + 1, col0:col0 + C]
    assert x.stride() == (5 * C, 1) and w.stride() == (C + 16, 1)
    return x, w


@pytest.mark.parametrize("dtname", list(DTYPES))
@pytest.mark.parametrize("B,C,V", LOGIT_SHAPES)
def test_last_logits_against_float64(B, C, V, dtname):
    from fastmax_experiments_amd.generate import last_logits
    dt = DTYPES[dtname]
    x, w = _logit_operands(B, C, V, dt)
    x64, w64 = x.double().cpu().numpy(), w.double().cpu().numpy()
    want = x64 @ w64.T
    bound = (C + 3) * 2.0 ** -24 * (np.abs(x64) @ np.abs(w64).T)
    for out_dt in dict.fromkeys((torch.float32, dt)):
        got = last_logits(x, w, out_dt)
        assert got.shape == (B, V) and got.dtype == out_dt
        err = np.abs(got.double().cpu().numpy() - want)
        limit = bound + OUT_ROUNDING[out_dt] * (np.abs(want) + bound)
        print(f"last_logits {dtname} -> {out_dt} B={B} C={C} V={V}: worst err / bound {float((err / limit).max()):.3f}")
        assert (err <= limit).all()
        assert torch.equal(got, last_logits(x, w, out_dt)), "two calls differ"


@pytest.mark.parametrize("dtname", list(DTYPES))
def test_a_rows_logits_do_not_depend_on_its_batch(dtname):
    from fastmax_experiments_amd.generate import last_logits
    x, w = _logit_operands(17, 2056, 257, DTYPES[dtname])
    batch = last_logits(x, w)
    for b in range(17):
        assert torch.equal(batch[b:b + 1], last_logits(x[b:b + 1], w)), f"row {b} alone differs from row {b} of the batch"
    assert torch.equal(batch[3:8], last_logits(x[3:8], w))


@pytest.mark.parametrize("dtname", list(DTYPES))
@pytest.mark.parametrize("B,C,V", [(3, 2056, 257), (9, 96, 63)])
def test_sixteen_byte_route_and_element_route_give_equal_bits(B, C, V, dtname):
    from fastmax_experiments_amd.generate import last_logits
    dt = DTYPES[dtname]
    x, w = _logit_operands(B, C, V, dt)                           # columns from 8: whole 16-byte pieces
    _, w_off = _logit_operands(B, C, V, dt, col0=1)               # columns from 1: no 16-byte boundary
    w_off.copy_(w)
    assert w.data_ptr() % 16 == 0 and w_off.data_ptr() % 16 != 0 and torch.equal(w, w_off)
    assert torch.equal(last_logits(x, w), last_logits(x, w_off))


@pytest.mark.parametrize("dtname", list(DTYPES))
def test_last_logits_keep_the_recorded_bits(dtname):
    """tests/golden/make_golden_last_logits.py: both load routes, G = 1, 2, 4 and 8 + 1, both output types, with and without a
    bias, against the bits a build before the plain and the biased entry point shared a kernel produced"""
    from fastmax_experiments_amd.generate import last_logits
    dt = DTYPES[dtname]
    d, m = load_golden(f"last_logits_{dtname}")

    def tensor(a, dtype):
        t = torch.from_numpy(a)
        return (t.view(dtype) if t.dtype == torch.int16 else t).cuda()
    V, C = m["V"], m["C_elem"]
    bias = tensor(d["bias"], dt)
    cases = {"vec": (tensor(d["vec_x"], dt), tensor(d["vec_w"], dt)),
             "elem": (tensor(d["elem_hidden"], dt)[:, -1], tensor(d["elem_wide"], dt)[1:V + 1, 1:1 + C])}
    assert cases["vec"][1].shape == (V, m["C_vec"]) and cases["elem"][1].stride() == (120, 1) and cases["elem"][0].stride() == (5 * C, 1)
    assert bias.shape == (V + 5,) and m["batches"] == [1, 2, 3, 9]
    for case, (x, w) in cases.items():
        for B in m["batches"]:
            for out_name, out_dt in (("f32", torch.float32), ("same", dt)):
                for bias_name, b in (("bias", bias), ("nobias", None)):
                    want = tensor(d[f"{case}_B{B}_{out_name}_{bias_name}"], out_dt)
                    got = last_logits(x[:B], w, out_dt, bias=b)
                    assert got.dtype == want.dtype and torch.equal(got, want), (case, B, out_name, bias_name)


# ---- 2. the keep mask ------------------------------------------------------------------------------------------------------------
def _sampler(seed=77):
    from fastmax_experiments_amd.generate import Sampler
    return Sampler(seed)


@pytest.mark.parametrize("k", [1, 5, 11, 12, 17])
def test_keep_mask_on_designed_ties(k):
    rows = np.stack([r for _, r in tie_cases()]).astype(np.float32)
    got = _sampler().keep_mask(torch.from_numpy(rows).cuda(), k)
    assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), ref.keep_mask(rows, k))


@pytest.mark.parametrize("V", [1, 7, 256, 257, 4099])
def test_keep_mask_on_random_rows(V):
    g = np.random.default_rng(V)
    fine = g.normal(0, 3, (3, V))
    coarse = np.round(g.normal(0, 3, (3, V)) * 2) / 2             # multiples of 0.5: many ties, +0.0 and -0.0 among them
    rows = np.concatenate([fine, coarse, -np.abs(coarse) * 0.0 + np.where(coarse > 4, 1.0, 0.0)]).astype(np.float32)
    rows[1, ::5] = -np.inf
    dev = torch.from_numpy(rows).cuda()
    s = _sampler()
    for k in sorted({k for k in (1, 2, 200, V - 1, V) if k >= 1}):
        want = ref.keep_mask(rows, k)
        assert (want.sum(1) == min(k, V)).all()
        assert np.array_equal(s.keep_mask(dev, k).cpu().numpy(), want), f"V={V} k={k}"
    assert s.keep_mask(dev, None).all() and s.draws == 0


# ---- 3. greedy -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_k", [None, 1, 50])
def test_temperature_zero_is_argmax_with_the_lowest_index_on_ties(top_k):
    g = np.random.default_rng(11)
    rows = g.normal(0, 3, (6, 515)).astype(np.float32)
    rows[2, [400, 17, 203]] = rows[2].max() + 1.0                 # the maximum three times: index 17 wins
    rows[4, :] = -2.5                                             # one value everywhere: index 0
    s = _sampler()
    got = s.sample(torch.from_numpy(rows).cuda(), temperature=0.0, top_k=top_k)
    assert got.dtype == torch.int64 and got.shape == (6,) and got.is_cuda and s.draws == 1
    want = rows.argmax(1)
    assert want[2] == 17 and want[4] == 0 and np.array_equal(got.cpu().numpy(), want)


# ---- 4. sampling -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,k,temperature,draws", [(515, 50, 0.8, 8), (4099, 200, 0.8, 8), (515, None, 0.1, 8), (7, 3, 0.5, 8),
                                                   (32000, 200, 0.8, 1)])
def test_sampled_tokens_match_the_restatement(V, k, temperature, draws):
    B, seed = 64, 2 ** 40 + 9
    rows = np.random.default_rng(V).normal(0, 3, (B, V)).astype(np.float32)
    dev = torch.from_numpy(rows).cuda()
    s = _sampler(seed)
    got = []
    for d in range(draws):
        assert s.draws == d
        got.append(s.sample(dev, temperature, k).cpu().numpy())
    compared = mismatched = 0
    for d in range(draws):
        want, gap = ref.sample(rows, temperature, k, seed, d)
        assert (got[d] >= 0).all() and (got[d] < V).all()
        assert ref.keep_mask(rows, k)[np.arange(B), got[d]].all(), "a token outside the kept set"
        clear = gap >= 1e-3
        compared += int(clear.sum())
        mismatched += int((got[d][clear] != want[clear]).sum())
    skipped = B * draws - compared
    print(f"sample V={V} k={k} T={temperature}: {compared} compared, {skipped} closer than 1e-3, {mismatched} mismatched")
    assert mismatched == 0
    assert skipped <= 0.01 * B * draws
    # the same seed and draw: the same tokens; the next draw: other tokens somewhere
    again = _sampler(seed)
    again.draws = draws - 1
    assert np.array_equal(again.sample(dev, temperature, k).cpu().numpy(), got[-1])
    assert again.draws == draws
    assert not np.array_equal(again.sample(dev, temperature, k).cpu().numpy(), got[-1])


# ---- 5. generate -----------------------------------------------------------------------------------------------------------------
VOCAB, PROMPT, NEW = 515, 5, 8


@pytest.fixture(scope="module", params=["fastmax", "linearmax"])
def model(request):
    from fastmax_experiments_amd.attention_block import build_rope_cache
    from fastmax_experiments_amd.block import Block, BlockStack
    from fastmax_experiments_amd.generate import NextTokenHead
    alg = request.param
    torch.manual_seed(3)
    stack = BlockStack([Block.from_config("pythia-14m", attn_alg=alg) for _ in range(2)]).cuda().eval()
    head = NextTokenHead(128, VOCAB).cuda().eval()
    wte = torch.randn(VOCAB, 128).cuda()
    cos, sin = build_rope_cache(PROMPT + NEW, stack.blocks[0].attn.rope_n_elem, device="cuda")
    prompt = torch.randint(0, VOCAB, (2, PROMPT), generator=torch.Generator().manual_seed(4)).cuda()
    return dict(alg=alg, stack=stack, head=head, wte=wte, cos=cos, sin=sin, prompt=prompt)


def _states(alg, B=2):
    from fastmax_experiments_amd.decode import FastmaxDecodeState, LinearmaxDecodeState
    if alg == "fastmax":
        return [FastmaxDecodeState(B, 4, 32, "cuda", p=2, n_query_groups=4) for _ in range(2)]
    return [LinearmaxDecodeState(B, 4, 32, "cuda", n_query_groups=4) for _ in range(2)]


def _generate(m, prompt=None, **kw):
    from fastmax_experiments_amd.generate import generate
    prompt = m["prompt"] if prompt is None else prompt
    return generate(m["wte"], m["stack"], m["head"], _states(m["alg"]), prompt, PROMPT + NEW, cos=m["cos"], sin=m["sin"], **kw)


def test_greedy_generate_is_the_argmax_of_its_own_logits(model):
    m = model
    out = _generate(m, temperature=0.0)
    assert out.shape == (2, PROMPT + NEW) and out.dtype == torch.int64 and torch.equal(out[:, :PROMPT], m["prompt"])
    assert int(out.min()) >= 0 and int(out.max()) < VOCAB
    # generate's own output through fresh states and the same modules: the prompt, then token by token
    states = _states(m["alg"])
    pos = torch.arange(PROMPT + NEW, device="cuda")
    with torch.no_grad():
        for a, b in [(0, PROMPT)] + [(t, t + 1) for t in range(PROMPT, PROMPT + NEW - 1)]:
            x = torch.nn.functional.embedding(out[:, a:b], m["wte"])
            h = m["stack"](x, m["cos"][a:b], m["sin"][a:b], pos[a:b], states)
            logits = m["head"].logits(h)
            assert logits.shape == (2, VOCAB) and logits.dtype == torch.float32
            assert torch.equal(logits.argmax(-1), out[:, b]), f"position {b}"


def test_sampled_generate_reproduces_under_its_seed(model):
    from fastmax_experiments_amd.generate import Sampler
    a = _generate(model, temperature=1.0, top_k=100, sampler=Sampler(21))
    b = _generate(model, temperature=1.0, top_k=100, sampler=Sampler(21))
    c = _generate(model, temperature=1.0, top_k=100, sampler=Sampler(22))
    assert a.shape == (2, PROMPT + NEW) and torch.equal(a, b) and not torch.equal(a, c)
    s = Sampler(21)
    _generate(model, temperature=1.0, sampler=s)
    assert s.draws == NEW


@pytest.mark.parametrize("rows", ["two_prompts", "one_prompt_twice"])
def test_generate_stops_once_every_row_has_produced_eos(model, rows):
    """eos_id = the first generated token of row 0.  With the same prompt in both rows both produce it at once and the loop
    ends after one token; with two prompts it ends where the greedy run without eos_id says every row has produced it."""
    prompt = model["prompt"] if rows == "two_prompts" else model["prompt"][:1].expand(2, PROMPT).contiguous()
    full = _generate(model, prompt, temperature=0.0)
    eos = int(full[0, PROMPT])
    hit = (full[:, PROMPT:] == eos).cpu().numpy()
    done = np.logical_or.accumulate(hit, axis=1).all(axis=0)
    n = PROMPT + (int(np.argmax(done)) + 1 if done.any() else NEW)
    if rows == "one_prompt_twice":
        assert n == PROMPT + 1
    out = _generate(model, prompt, temperature=0.0, eos_id=eos)
    assert out.shape == (2, n) and torch.equal(out, full[:, :n])
    if n < PROMPT + NEW:
        assert (out[:, PROMPT:] == eos).any(dim=1).all()
