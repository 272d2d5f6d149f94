"""Top-p (nucleus) sampling on an MI355X (csrc/next_token_sample.h: select_nucleus; generate.Sampler / DecodeCursor /
GraphedDecoder / generate with ``top_p``) against the float64 restatement (nucleus_ref.py).

The band.  The kept set must be EXACTLY a prefix of the row's order (key descending, index ascending) inside the top-k's
candidates, on every row, and its length n must satisfy C(n) >= top_p - eps and C(n - 1) < top_p + eps with C from float64 and
eps = nucleus_ref.epsilon(V) = 2.02 (2^-23 ln V + 2^-22 + V 2^-40): the kernel evaluates C with float32 weights
w = expf((logit - m) / T) -- two roundings in the argument, relative 2^-23 |x| each entry, which summed against the
probabilities is at most 2^-23 ln V (an entropy); expf within 2 ulp; a truncation to 2^-40 per entry against a total >= 1 -- in
exact integer sums, and the error enters numerator and denominator of C (the factor 2).  That is 2.5e-6 at V = 4099 and 3.2e-6 at
V = 50304, below 2^-18; test_nucleus_cpu.py shows that this band pins n to one value on more than 99 % of the sharp group's rows.

1. the mask against the band: the sharp group, top_p 0.95 / 0.999 at temperature 2 at every V, designed ties (exact);
2. a row's kept set alone, in a batch, on a second call, under another row stride and on the unaligned route: equal bits; every
   token ``sample`` returns lies inside the mask;
3. top_p = 1.0 and None: the existing sampler's tokens and draw count;
4. top_p = 1e-9: the temperature-0 tokens;
5. tokens against the restated scores over the kernel's own (band-checked) mask wherever the float64 gap is >= 1e-3
   (test_next_token_gpu's rule: at most 1 % of the cases may be closer);
6. the cursor's draws against the sampler's;
7. generate through two pythia-14m blocks: reproduces under its seed; the graphed loop equals the eager one bit for bit."""
import numpy as np
import pytest
import torch

import nucleus_ref as nuc
from test_cursor_gpu import NEW, PROMPT, _decoder, _eager, _model, _states

pytestmark = pytest.mark.gpu

ALL_V = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4099, 50304]
SHARP = [(p, t, k) for p in (0.1, 0.5, 0.9) for t in (0.5, 1.0) for k in (None, 1, 50)]
WIDE = [(p, 2.0, k) for p in (0.95, 0.999) for k in (None, 50)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from fastmax_experiments_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _sampler(seed=77):
    from fastmax_experiments_amd.generate import Sampler
    return Sampler(seed)


def _on_device(rows, aligned=True, pad=4):
    """rows as a view with a row stride > V: every row base on a 16-byte boundary, or none of them"""
    B, V = rows.shape
    stride = (V + 3) // 4 * 4 + pad                               # whole 16-byte pieces
    flat = torch.zeros(B * stride + 4, dtype=torch.float32, device="cuda")
    off = 0 if aligned else 1
    view = flat[off:off + B * stride].view(B, stride)[:, :V]
    view.copy_(torch.from_numpy(rows))
    assert view.stride() == (stride, 1) and stride > V
    assert all(((view.data_ptr() + 4 * b * stride) % 16 == 0) == aligned for b in range(B))
    return view


class Band:
    """checks masks against the restatement, row by row, and keeps the worst figures"""

    def __init__(self):
        self.rows = self.pinned = 0
        self.low = self.high = -np.inf          # worst top_p - C(n) and worst C(n - 1) - top_p: both stay below eps

    def check(self, rows, mask, k, p, t, what):
        eps = nuc.epsilon(rows.shape[1])
        for b, row in enumerate(rows):
            idx, C = nuc.cumulative(row, k, t)
            n = nuc.prefix_length(mask[b], idx)
            assert n is not None and n >= 1, f"{what} row {b}: the kept set is not a prefix of the order"
            lo, hi = nuc.band(C, p, eps)
            p32 = float(np.float32(p))
            if n < len(C):
                self.low = max(self.low, p32 - C[n - 1])
            if n > 1:
                self.high = max(self.high, C[n - 2] - p32)
            assert lo <= n <= hi, f"{what} row {b}: n = {n}, the band allows {lo} .. {hi} (exact {nuc.length(C, p)})"
            self.rows += 1
            self.pinned += lo == hi

    def report(self, what):
        print(f"{what}: {self.rows} rows, {self.pinned} pinned to one length; worst top_p - C(n) = {self.low:.3e}, "
              f"worst C(n - 1) - top_p = {self.high:.3e} (both must stay below eps)")


# ---- 1. the mask against the band ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", ALL_V)
def test_the_mask_is_a_prefix_of_the_order_inside_the_band(V):
    """B = 1, 3 and 9 fine and as many rounded rows, B = 3 also from row bases off the 16-byte grid: 32 rows a case.  Up to
    V = 4099 the sharp group, where the band must pin the length on at least 99 % of the rows; above, two of its cases."""
    s, sharp, wide = _sampler(), Band(), Band()
    cases = [(c, sharp) for c in (SHARP if V <= 4099 else [(0.9, 1.0, None), (0.9, 0.5, 50)])] + [(c, wide) for c in WIDE]
    for B, aligned in ((1, True), (3, True), (3, False), (9, True)):
        rows = nuc.rows(V, B)
        dev = _on_device(rows, aligned)
        for (p, t, k), band in cases:
            mask = s.keep_mask(dev, k, top_p=p, temperature=t)
            assert mask.dtype == torch.bool and mask.shape == rows.shape
            band.check(rows, mask.cpu().numpy(), k, p, t, f"V={V} B={B} aligned={aligned} top_p={p} T={t} k={k}")
    sharp.report(f"V={V} eps={nuc.epsilon(V):.3e} sharp group")
    wide.report(f"V={V} top_p 0.95 / 0.999 at temperature 2")
    assert s.draws == 0 and sharp.rows == 32 * (len(cases) - len(WIDE)) and wide.rows == 32 * len(WIDE)
    if V <= 4099:
        assert sharp.pinned >= 0.99 * sharp.rows


@pytest.mark.parametrize("V", [5, 8, 12])
def test_designed_ties_keep_the_lowest_indices(V):
    rows = nuc.tie_rows(V)
    dev = _on_device(rows)
    s = _sampler()
    for p in (0.3, 0.6, 0.85):
        for k in (None, 3):
            got = s.keep_mask(dev, k, top_p=p).cpu().numpy()
            assert np.array_equal(got, nuc.keep_mask(rows, k, p, 1.0)), (V, p, k)


# ---- 2. one row, many ways -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,k,p,t", [(257, None, 0.9, 1.0), (4099, 50, 0.5, 0.5), (1025, None, 0.999, 2.0)])
def test_a_rows_kept_set_depends_on_the_row_alone(V, k, p, t):
    rows = nuc.rows(V, 9)
    s = _sampler()
    batch = s.keep_mask(_on_device(rows), k, top_p=p, temperature=t)
    assert torch.equal(batch, s.keep_mask(_on_device(rows), k, top_p=p, temperature=t)), "two calls differ"
    assert torch.equal(batch, s.keep_mask(_on_device(rows, pad=12), k, top_p=p, temperature=t)), "another row stride"
    assert torch.equal(batch, s.keep_mask(_on_device(rows, aligned=False), k, top_p=p, temperature=t)), "the unaligned route"
    assert torch.equal(batch, s.keep_mask(torch.from_numpy(rows).cuda(), k, top_p=p, temperature=t)), "contiguous rows"
    for b in (0, 8, 9, 17):
        alone = s.keep_mask(_on_device(rows[b:b + 1]), k, top_p=p, temperature=t)
        assert torch.equal(alone[0], batch[b]), f"row {b} alone"
    # what sample draws from: every token of several draws lies inside the mask, on both routes
    mask = batch.cpu().numpy()
    for aligned in (True, False):
        dev = _on_device(rows, aligned)
        for d in range(6):
            tok = s.sample(dev, t, k, top_p=p).cpu().numpy()
            assert mask[np.arange(len(rows)), tok].all(), f"draw {d}: a token outside the nucleus"
    assert s.draws == 12


# ---- 3. the off switch -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,k,t", [(515, 50, 0.8), (4099, None, 1.0), (7, 3, 0.5)])
def test_top_p_one_and_none_are_the_existing_sampler(V, k, t):
    dev = _on_device(np.random.default_rng(V).normal(0, 3, (16, V)).astype(np.float32))
    plain, one, none = _sampler(9), _sampler(9), _sampler(9)
    for d in range(4):
        want = plain.sample(dev, t, k)
        assert torch.equal(one.sample(dev, t, k, top_p=1.0), want) and torch.equal(none.sample(dev, t, k, top_p=None), want)
        assert plain.draws == one.draws == none.draws == d + 1
    assert torch.equal(plain.keep_mask(dev, k), one.keep_mask(dev, k, top_p=1.0, temperature=t))
    # a nucleus that keeps all of K (top_p next to 1 on a flat row) draws the top-k sampler's token too
    flat = torch.zeros(4, V, device="cuda")
    assert one.keep_mask(flat, k, top_p=0.9999999, temperature=t).sum(1).tolist() == [min(k or V, V)] * 4
    assert torch.equal(one.sample(flat, t, k, top_p=0.9999999), plain.sample(flat, t, k))


# ---- 4. a nucleus of one -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_k", [None, 1, 50])
def test_a_tiny_top_p_is_the_argmax_with_the_lowest_index_on_ties(top_k):
    g = np.random.default_rng(11)
    rows = g.normal(0, 3, (6, 515)).astype(np.float32)
    rows[2, [400, 17, 203]] = rows[2].max() + 1.0                 # the maximum three times: index 17 wins
    rows[4, :] = -2.5                                             # one value everywhere: index 0
    dev = _on_device(rows)
    s = _sampler()
    greedy = s.sample(dev, temperature=0.0, top_k=top_k)
    for d in range(3):
        assert torch.equal(s.sample(dev, temperature=0.8, top_k=top_k, top_p=1e-9), greedy)
    want = rows.argmax(1)
    assert want[2] == 17 and want[4] == 0 and np.array_equal(greedy.cpu().numpy(), want)
    assert s.keep_mask(dev, top_k, top_p=1e-9, temperature=0.8).sum(1).tolist() == [1] * 6
    # temperature 0 ignores top_p: the argmax, and the mask is the top-k's
    assert torch.equal(s.sample(dev, temperature=0.0, top_k=top_k, top_p=0.3), greedy)
    assert torch.equal(s.keep_mask(dev, top_k, top_p=0.3, temperature=0.0), s.keep_mask(dev, top_k))


# ---- 5. sampling -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,k,top_p,temperature,draws", [(515, 50, 0.9, 0.8, 8), (4099, 200, 0.9, 0.8, 8), (515, None, 0.5, 0.1, 8),
                                                         (7, 3, 0.7, 0.5, 8), (32000, 200, 0.9, 0.8, 1)])
def test_sampled_tokens_match_the_restatement_inside_the_kernels_mask(V, k, top_p, temperature, draws):
    B, seed = 64, 2 ** 40 + 9
    rows = np.random.default_rng(V).normal(0, 3, (B, V)).astype(np.float32)
    dev = torch.from_numpy(rows).cuda()
    s = _sampler(seed)
    mask = s.keep_mask(dev, k, top_p=top_p, temperature=temperature).cpu().numpy()
    band = Band()
    band.check(rows, mask, k, top_p, temperature, f"V={V}")
    band.report(f"V={V} k={k} top_p={top_p} T={temperature}")
    assert (mask.sum(1) < min(k or V, V)).any(), "the nucleus never cut anything: the case shows nothing"
    got = []
    for d in range(draws):
        assert s.draws == d
        got.append(s.sample(dev, temperature, k, top_p=top_p).cpu().numpy())
    compared = mismatched = 0
    for d in range(draws):
        want, gap = nuc.sample_in(mask, rows, temperature, seed, d)
        assert (got[d] >= 0).all() and (got[d] < V).all()
        assert mask[np.arange(B), got[d]].all(), "a token outside the kept set"
        clear = gap >= 1e-3
        compared += int(clear.sum())
        mismatched += int((got[d][clear] != want[clear]).sum())
    skipped = B * draws - compared
    print(f"sample V={V} k={k} top_p={top_p} T={temperature}: {compared} compared, {skipped} closer than 1e-3, {mismatched} mismatched")
    assert mismatched == 0
    assert skipped <= 0.01 * B * draws
    again = _sampler(seed)
    again.draws = draws - 1
    assert np.array_equal(again.sample(dev, temperature, k, top_p=top_p).cpu().numpy(), got[-1]) and again.draws == draws


# ---- 6. the cursor -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_draw", [0, 2 ** 32 - 2], ids=["from0", "carry"])
@pytest.mark.parametrize("V,k,top_p,temperature", [(515, 50, 0.9, 0.8), (7, 3, 0.7, 0.5), (515, None, 0.5, 1.0), (515, 50, 0.3, 0.0)])
def test_cursor_draws_equal_the_samplers_at_the_same_draw_numbers(V, k, top_p, temperature, first_draw):
    from fastmax_experiments_amd.generate import DecodeCursor, Sampler
    B, seed, draws, pos0 = 64, 2 ** 40 + 9, 8, 3
    logits = torch.from_numpy(np.random.default_rng(V).normal(0, 3, (B, V)).astype(np.float32)).cuda()
    s = Sampler(seed)
    s.draws = first_draw
    want = torch.stack([s.sample(logits, temperature, k, top_p=top_p) for _ in range(draws)], dim=1)          # (B, draws)
    if temperature > 0:
        assert not torch.equal(want[:, 0], want[:, 1])
        plain = Sampler(seed)
        plain.draws = first_draw
        assert not torch.equal(plain.sample(logits, temperature, k), want[:, 0]), "the nucleus changed no token"
    eos = int(want[0, 0])
    cursor = DecodeCursor("cuda")
    cursor.arm(pos0, first_draw, seed)
    tok = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    out = torch.full((B, pos0 + 1 + draws), -1, dtype=torch.int64, device="cuda")
    done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    wte, rope = torch.zeros(4, 8, device="cuda"), torch.zeros(out.shape[1], 8, device="cuda")
    x, row = torch.zeros(B, 8, device="cuda"), torch.zeros(2, 1, 8, device="cuda")
    for d in range(draws):
        cursor.feed(torch.zeros(B, dtype=torch.int64, device="cuda"), wte, x, rope, rope, row[0], row[1])
        cursor.sample(logits, tok, out, done, eos, temperature, k, top_p=top_p)
        assert cursor.read() == dict(pos=pos0 + d + 1, next=pos0 + d + 1, overflow=False)
        assert torch.equal(tok, want[:, d]), f"draw {first_draw + d}"
        assert torch.equal(done.bool(), (want[:, :d + 1] == eos).any(dim=1))
    assert torch.equal(out[:, pos0 + 1:], want) and bool((out[:, :pos0 + 1] == -1).all())


# ---- 7. generate -------------------------------------------------------------------------------------------------------------------
KW = dict(top_p=0.9, top_k=50, temperature=0.8)


@pytest.mark.parametrize("name", ["fastmax", "linearmax"])
def test_generate_with_top_p_reproduces_under_its_seed(name):
    from fastmax_experiments_amd.generate import Sampler
    m = _model(name)
    s = Sampler(21)
    a = _eager(m, _states(m), m["prompt"], PROMPT + NEW, sampler=s, **KW)
    b = _eager(m, _states(m), m["prompt"], PROMPT + NEW, sampler=Sampler(21), **KW)
    c = _eager(m, _states(m), m["prompt"], PROMPT + NEW, sampler=Sampler(22), **KW)
    plain = _eager(m, _states(m), m["prompt"], PROMPT + NEW, sampler=Sampler(21), top_k=50, temperature=0.8)
    assert a.shape == (2, PROMPT + NEW) and torch.equal(a[:, :PROMPT], m["prompt"]) and s.draws == NEW
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert not torch.equal(a, plain), "top_p changed no token"


@pytest.mark.parametrize("with_eos", [False, True], ids=["no-eos", "eos"])
@pytest.mark.parametrize("name", ["fastmax", "linearmax", "neox"])
def test_graphed_generate_with_top_p_equals_the_eager_loop(name, with_eos):
    from fastmax_experiments_amd.generate import Sampler, generate
    m = _model(name)
    kw = dict(KW)
    if with_eos:                                                  # a token row 0 produces on the way
        kw["eos_id"] = int(_eager(m, _states(m), m["prompt"], PROMPT + NEW, sampler=Sampler(21), **KW)[0, PROMPT + 2])
    eager_states, states = _states(m), _states(m)
    decoder = _decoder(m, states, **kw)
    decoder.poll = 1                                              # with an eos the caches stop where the eager loop's stop
    s_eager, s_graph = Sampler(21), Sampler(21)
    want = _eager(m, eager_states, m["prompt"], PROMPT + NEW, sampler=s_eager, **kw)
    got = generate(m["wte"], m["stack"], m["head"], states, m["prompt"], PROMPT + NEW, cos=m["cos"], sin=m["sin"], sampler=s_graph,
                   graphed=decoder, **kw)
    assert got.shape == want.shape and torch.equal(got, want)
    assert s_graph.draws == s_eager.draws == want.shape[1] - PROMPT
    for a, b in zip(states, eager_states):
        assert a.count == b.count == want.shape[1] - 1 and torch.equal(a.state, b.state)
    assert decoder.captures == 1 and decoder.replays == want.shape[1] - PROMPT - 1
    assert not decoder.cursor.read()["overflow"]
    for other in (dict(kw, top_p=0.8), {k: v for k, v in kw.items() if k != "top_p"}, dict(kw, top_p=1.0)):
        with pytest.raises(ValueError, match="graphed was built from other"):
            generate(m["wte"], m["stack"], m["head"], states, m["prompt"], PROMPT + NEW, cos=m["cos"], sin=m["sin"], graphed=decoder,
                     **other)
