"""Top-p (nucleus) sampling (include/fastmax_hip_nucleus.h, csrc/next_token_sample.h, fastmax_experiments_amd/generate.py),
everything that needs no device:

1. the sources and the shared sampler header in the build's lists (the binding table against this header, and its rows against
   the samplers' without top_p: test_binding_cpu);
2. every rejection the header adds, returned before any launch;
3. the host contract: a top_p outside (0, 1] raises ValueError everywhere before any device work, CPU tensors raise the existing
   RuntimeError, ``serves`` tells two top_p apart;
4. the restatement (nucleus_ref.py): designed rows, the tensor-op route's keep rule (torch sort + cumsum in float64), the
   library's fixed-point evaluation restated in numpy inside the band of nucleus_ref.epsilon, how sharp that band is, and the
   distribution of the restated draw inside a nucleus."""

import numpy as np
import pytest
import torch

import next_token_ref as ref
import nucleus_ref as nuc
from fastmax_experiments_amd import _lib, build, generate
from test_next_token_cpu import CHI2_999_DF7, LOGITS8, SEEDS, _chi2

BAD_TOP_P = [0, -0.1, 1.5, float("nan")]


# ---- 1. the build ------------------------------------------------------------------------------------------------------------
def test_the_build_watches_the_header():
    assert "next_token.hip" in build.SOURCES and "decode_cursor.hip" in build.SOURCES and "next_token_sample.h" in build.HEADERS


# ---- 2. rejections -----------------------------------------------------------------------------------------------------------
A = 0x10000          # a made-up address, 16-byte aligned: every call below is refused before anything could touch it


def _sample(**over):
    a = dict(logits=A, ld=515, tokens=A, B=2, V=515, top_k=50, top_p=0.9, temperature=0.8, seed=77, draw=0, stream=None)
    a.update(over)
    return _lib.lib().fastmax_hip_sample_nucleus(*a.values())


def _mask(**over):
    a = dict(logits=A, ld=515, mask=A, ldm=515, B=2, V=515, top_k=50, top_p=0.9, temperature=0.8, stream=None)
    a.update(over)
    return _lib.lib().fastmax_hip_nucleus_mask(*a.values())


def _cursor(**over):
    a = dict(logits=A, ld=515, cursor=A, tok=A, out=A, ldo=13, L=13, done=A, eos_id=-1, B=2, V=515, top_k=50, temperature=0.8,
             top_p=0.9, stream=None)
    a.update(over)
    return _lib.lib().fastmax_hip_sample_cursor_nucleus(*a.values())


def test_the_entry_points_reject_bad_calls_before_any_launch():
    big = _lib.NUCLEUS_MAX_V + 1
    assert _lib.NUCLEUS_MAX_V == nuc.MAX_V >= 262144
    for call in (_sample, _mask, _cursor):
        for p in BAD_TOP_P + [1.0000001, -1.0, float("inf")]:
            assert call(top_p=p) == _lib.E_BAD_SHAPE, (call.__name__, p)
        for t in (-0.5, float("nan"), float("inf")):
            assert call(temperature=t) == _lib.E_BAD_SHAPE, (call.__name__, t)
        for bad in (dict(V=0), dict(B=0), dict(top_k=-1), dict(ld=514), dict(V=big, ld=big)):
            assert call(**dict(bad, ldm=big) if call is _mask else bad) == _lib.E_BAD_SHAPE, (call.__name__, bad)
        assert call(logits=None) == _lib.E_NULL and call(logits=A + 2) == _lib.E_ALIGNMENT
    assert _sample(tokens=None) == _lib.E_NULL and _sample(tokens=A + 4) == _lib.E_ALIGNMENT
    assert _mask(mask=None) == _lib.E_NULL and _mask(ldm=514) == _lib.E_BAD_SHAPE
    for missing in ("cursor", "tok", "out"):
        assert _cursor(**{missing: None}) == _lib.E_NULL, missing
    assert _cursor(done=None, eos_id=3) == _lib.E_NULL and _cursor(L=0) == _lib.E_BAD_SHAPE and _cursor(ldo=12) == _lib.E_BAD_SHAPE
    assert _cursor(cursor=A + 4) == _lib.E_ALIGNMENT and _cursor(tok=A + 4) == _lib.E_ALIGNMENT and _cursor(out=A + 4) == _lib.E_ALIGNMENT


# ---- 3. the host contract ------------------------------------------------------------------------------------------------------
class _State:
    """stands for a decode state cache where nothing is run"""
    B, count = 2, 0


@pytest.mark.parametrize("top_p", BAD_TOP_P)
def test_a_top_p_outside_its_range_raises_before_any_device_work(top_p):
    from fastmax_experiments_amd.block import Block
    logits = torch.zeros(2, 8)               # CPU tensors: a call would raise RuntimeError, the argument checks come first
    s = generate.Sampler(seed=5)
    with pytest.raises(ValueError, match="top_p"):
        s.sample(logits, top_p=top_p)
    with pytest.raises(ValueError, match="top_p"):
        s.keep_mask(logits, 3, top_p=top_p)
    assert s.draws == 0
    head = generate.NextTokenHead(16, 40)
    with pytest.raises(ValueError, match="top_p"):
        head(torch.zeros(2, 3, 16), s, top_p=top_p)
    kw = dict(cos=torch.zeros(8, 4), sin=torch.zeros(8, 4))
    with pytest.raises(ValueError, match="top_p"):
        generate.generate(torch.zeros(40, 16), [], head, [], torch.zeros(2, 3, dtype=torch.int64), 6, top_p=top_p, **kw)
    cursor = object.__new__(generate.DecodeCursor)          # no record: the check comes before anything reads one
    with pytest.raises(ValueError, match="top_p"):
        cursor.sample(logits, torch.zeros(2, dtype=torch.int64), torch.zeros(2, 4, dtype=torch.int64), top_p=top_p)
    with pytest.raises(ValueError, match="top_p"):
        generate.GraphedDecoder(torch.zeros(40, 128), [Block.from_config("pythia-14m")], generate.NextTokenHead(128, 40), [_State()],
                                cos=torch.zeros(8, 8), sin=torch.zeros(8, 8), max_len=9, top_p=top_p)


def test_cpu_tensors_raise_the_existing_error_and_the_tensor_op_route_runs_anywhere():
    s = generate.Sampler(seed=5)
    logits = torch.zeros(2, 8)
    for p in (0.9, 1.0, None):
        with pytest.raises(RuntimeError, match="no CPU path"):
            s.sample(logits, top_p=p)
        with pytest.raises(RuntimeError, match="no CPU path"):
            s.keep_mask(logits, 3, top_p=p)
    assert s.draws == 0
    head = generate.NextTokenHead(16, 40)
    with pytest.raises(RuntimeError):
        head(torch.zeros(2, 3, 16), s, top_p=0.9)
    head.fused = False
    torch.manual_seed(0)
    x = torch.randn(64, 3, 16)
    tokens = head(x, None, temperature=0.8, top_k=5, top_p=0.5)
    assert tokens.shape == (64,)
    keep = nuc.keep_mask(head.logits(x).detach().numpy(), 5, 0.5, 0.8)
    assert keep[np.arange(64), tokens.numpy()].all() and (keep.sum(1) <= 5).all()
    # a nucleus of one entry is the argmax
    assert torch.equal(head(x, None, temperature=0.8, top_p=1e-9), head.logits(x).argmax(-1))


def test_serves_is_false_when_only_top_p_differs():
    d = object.__new__(generate.GraphedDecoder)
    g = dict(wte=object(), blocks=object(), head=object(), cos=object(), sin=object())
    d.given, d.states, d.temperature, d.top_k, d.eos_id, d.top_p = g, [], 0.8, 50, None, generate._nucleus(0.9)
    args = (g["wte"], g["blocks"], g["head"], [], g["cos"], g["sin"], 0.8, 50, None)
    assert d.serves(*args, 0.9) and d.serves(*args, top_p=0.9)
    assert not d.serves(*args) and not d.serves(*args, 0.8) and not d.serves(*args, 1.0) and not d.serves(*args, float("nan"))
    assert not d.serves(*(args[:6] + (0.7, 50, None)), 0.9)
    d.top_p = generate._nucleus(None)
    assert d.serves(*args) and d.serves(*args, 1.0) and d.serves(*args, None) and not d.serves(*args, 0.9)
    assert generate._nucleus(1.0) is None and generate._nucleus(None) is None and generate._nucleus(0.25) == 0.25


# ---- 4. the restatement --------------------------------------------------------------------------------------------------------
def test_restated_nucleus_on_designed_rows():
    a = np.array([[2.0, 0.0, 2.0, 0.0, -0.0, 2.0, 0.0, 1.0]], dtype=np.float32)          # order: 0 2 5 | 7 | 1 3 4 6
    w = np.exp(np.array([2.0, 2.0, 2.0, 1.0, 0, 0, 0, 0]))
    C = np.cumsum(w) / w.sum()
    idx, got = nuc.cumulative(a[0], None, 1.0)
    assert list(idx) == [0, 2, 5, 7, 1, 3, 4, 6] and np.allclose(got, C, rtol=0, atol=1e-15)
    assert 0.25 < C[0] < 0.3 < C[1] < 0.6 < C[2] < 0.85 < C[3] < 0.88 < C[4]
    for p, kept in ((0.25, [0]), (0.3, [0, 2]), (0.6, [0, 2, 5]), (0.85, [0, 2, 5, 7]), (0.88, [0, 1, 2, 5, 7]), (1e-9, [0])):
        assert list(np.nonzero(nuc.keep_mask(a, None, p, 1.0)[0])[0]) == kept, p
    assert list(np.nonzero(nuc.keep_mask(a, 2, 0.999, 1.0)[0])[0]) == [0, 2]                  # the top-k comes first
    assert list(np.nonzero(nuc.keep_mask(a, 4, 0.999, 1.0)[0])[0]) == [0, 2, 5, 7]
    assert list(np.nonzero(nuc.keep_mask(a, 4, 0.5, 0.25)[0])[0]) == [0, 2]                   # a colder row: C(2) = 2/3 of K
    for p in (None, 1.0):
        assert np.array_equal(nuc.keep_mask(a, 3, p, 1.0), ref.keep_mask(a, 3))
    assert np.array_equal(nuc.keep_mask(a, 3, 0.5, 0), ref.keep_mask(a, 3))                   # temperature 0: top_p is ignored
    for V in (5, 8, 12):
        for row in nuc.tie_rows(V):
            for k in (None, 3):
                C = nuc.cumulative(row, k, 1.0)[1]
                for p in (0.3, 0.6, 0.85):
                    assert np.abs(C - float(np.float32(p))).min() > 1e-3, (V, k, p)           # no C(j) meets a tested top_p


@pytest.mark.parametrize("top_k", [None, 1, 5])
def test_restatement_agrees_with_the_tensor_op_keep_rule(top_k):
    rows = np.concatenate([nuc.tie_rows(12), nuc.rows(12)])
    for t in (0.5, 1.0, 2.0):
        logits = torch.from_numpy(rows).double()
        if top_k is not None:
            keep = torch.from_numpy(ref.keep_mask(rows, top_k))          # the library's tie rule, which torch.topk leaves open
            logits = logits.masked_fill(~keep, float("-inf"))
        probs = torch.softmax(logits / float(np.float32(t)), dim=-1)
        for p in (0.1, 0.3, 0.6, 0.85, 0.95):
            got = generate._nucleus_keep(probs, float(np.float32(p))).numpy()
            assert np.array_equal(got, nuc.keep_mask(rows, top_k, p, t)), (t, p)


def test_fixed_point_evaluation_stays_inside_the_band_and_the_band_is_sharp():
    """The library's evaluation restated with numpy's float32 exp lands inside the band of nucleus_ref.epsilon on every row, and
    over the sharp group (V <= 4099, top_p 0.1 / 0.5 / 0.9, temperature 0.5 / 1, top_k None / 1 / 50) that band holds ONE
    length on at least 99 % of the rows: a wider epsilon would not pin the kernel down."""
    rows_seen = pinned = 0
    worst = 0.0
    for V in (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4099):
        assert nuc.epsilon(V) < 2.0 ** -18
        for row in np.concatenate([nuc.rows(V, B) for B in (1, 3, 9)]):
            for t in (0.5, 1.0):
                for k in (None, 1, 50):
                    idx, C = nuc.cumulative(row, k, t)
                    for p in (0.1, 0.5, 0.9):
                        lo, hi = nuc.band(C, p, nuc.epsilon(V))
                        assert lo <= nuc.length(C, p) <= hi
                        n = nuc.fixed_point_length(row, k, p, t)
                        assert lo <= n <= hi, (V, t, k, p, n, lo, hi)
                        worst = max(worst, abs(C[n - 1] - p) if n != nuc.length(C, p) else 0.0)
                        rows_seen += 1
                        pinned += lo == hi
    print(f"sharp group: {pinned} of {rows_seen} rows pinned to one length; worst |C(n) - top_p| where the fixed-point length "
          f"differs from the exact one: {worst:.3e}")
    assert pinned >= 0.99 * rows_seen


@pytest.mark.parametrize("seed", SEEDS)
def test_restated_draws_inside_a_nucleus_follow_the_renormalised_softmax(seed):
    """test_next_token_cpu's eight logits and four far smaller ones; top_p = 0.999 keeps exactly the eight (C(7) = 0.998): the
    draws over them follow their softmax renormalised, at 7 degrees of freedom"""
    n, t, p = 16384, 0.7, 0.999
    row = np.concatenate([LOGITS8, np.array([-6, -7, -8, -9], dtype=np.float32)])
    keep = nuc.keep_mask(row[None], None, p, t)[0]
    assert list(np.nonzero(keep)[0]) == list(range(8))
    z = LOGITS8.astype(np.float64) / float(np.float32(t))
    want = np.exp(z - z.max()) / np.exp(z - z.max()).sum()
    tokens, _ = nuc.sample_in(np.tile(keep, (n, 1)), np.tile(row, (n, 1)), t, seed, 0)
    assert (tokens < 8).all()
    x2 = _chi2(tokens, want)
    print(f"seed {seed}: chi-square {x2:.2f} (bound {CHI2_999_DF7})")
    assert x2 < CHI2_999_DF7
