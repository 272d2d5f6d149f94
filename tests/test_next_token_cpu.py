"""The next-token head (include/fastmax_hip_next_token.h, csrc/last_logits.hip, csrc/next_token.hip, fastmax_experiments_amd/generate.py), everything
that needs no device:

1. (the binding table against this header: test_binding_cpu);
2. every rejection the header lists, returned before any launch;
3. the restatement (next_token_ref.py): Philox-4x32-10 against its known-answer vectors, the keep mask on designed ties, and the
   distribution of the restated draws against softmax(logits / temperature);
4. the host contract of Sampler, NextTokenHead and generate: ValueErrors before any call, the seed taken from torch's generator."""

import numpy as np
import pytest
import torch

import next_token_ref as ref
from fastmax_experiments_amd import _lib, generate


# ---- 2. rejections -----------------------------------------------------------------------------------------------------------
A = 0x10000          # a made-up address, 16-byte aligned: every call below is refused before anything could touch it


def _logits(**over):
    a = dict(x=A, ldx=640, w=A, ldw=128, out=A, ldo=515, B=2, V=515, C=128, dtype=_lib.BF16, out_dtype=_lib.F32, stream=None)
    a.update(over)
    return _lib.lib().fastmax_hip_last_logits(*a.values())


def _sample(**over):
    a = dict(logits=A, ld=515, tokens=A, B=2, V=515, top_k=50, temperature=0.8, seed=77, draw=0, stream=None)
    a.update(over)
    return _lib.lib().fastmax_hip_sample(*a.values())


def _mask(**over):
    a = dict(logits=A, ld=515, mask=A, ldm=515, B=2, V=515, top_k=50, stream=None)
    a.update(over)
    return _lib.lib().fastmax_hip_topk_mask(*a.values())


def test_last_logits_rejects_bad_calls_before_any_launch():
    for missing in ("x", "w", "out"):
        assert _logits(**{missing: None}) == _lib.E_NULL, missing
    for dt in (-1, 3):
        assert _logits(dtype=dt) == _lib.E_BAD_DTYPE
    assert _logits(dtype=_lib.BF16, out_dtype=_lib.F16) == _lib.E_BAD_DTYPE
    assert _logits(dtype=_lib.F32, out_dtype=_lib.BF16) == _lib.E_BAD_DTYPE
    for bad in (dict(B=0), dict(V=0), dict(C=0), dict(B=-1), dict(V=-3), dict(ldw=127), dict(ldo=514), dict(ldx=-1),
                dict(C=2 ** 30 + 8, ldw=2 ** 30 + 8)):
        assert _logits(**bad) == _lib.E_BAD_SHAPE, bad
    assert _logits(x=A + 1) == _lib.E_ALIGNMENT and _logits(w=A + 1) == _lib.E_ALIGNMENT
    assert _logits(out=A + 2) == _lib.E_ALIGNMENT and _logits(dtype=_lib.F32, x=A + 2) == _lib.E_ALIGNMENT


def test_sample_and_mask_reject_bad_calls_before_any_launch():
    assert _sample(logits=None) == _lib.E_NULL and _sample(tokens=None) == _lib.E_NULL
    assert _mask(logits=None) == _lib.E_NULL and _mask(mask=None) == _lib.E_NULL
    for bad in (dict(V=0), dict(B=0), dict(top_k=-1), dict(ld=514), dict(V=2 ** 30 + 1, ld=2 ** 31)):
        assert _sample(**bad) == _lib.E_BAD_SHAPE, bad
        assert _mask(**dict(bad, ldm=max(bad.get("V", 515), 515))) == _lib.E_BAD_SHAPE, bad
    assert _mask(ldm=514) == _lib.E_BAD_SHAPE
    for t in (-0.5, float("nan"), float("inf")):
        assert _sample(temperature=t) == _lib.E_BAD_SHAPE, t
    assert _sample(logits=A + 2) == _lib.E_ALIGNMENT and _sample(tokens=A + 4) == _lib.E_ALIGNMENT
    assert _mask(logits=A + 2) == _lib.E_ALIGNMENT


# ---- 3. the restatement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
], ids=["zeros", "ones", "pi"])
def test_philox_known_answers(counter, key, want):
    got = ref.philox4x32_10([np.array([c], dtype=np.uint64) for c in counter], key)
    assert " ".join(f"{int(w[0]):08x}" for w in got) == want


def test_uniforms_are_exact_in_float32_and_strictly_inside_the_unit_interval():
    u = ref.uniforms(3, 4099, seed=2 ** 40 + 9, draw=5)
    assert u.shape == (3, 4099) and (u > 0).all() and (u < 1).all()
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    extremes = (np.array([0, 0xffffffff], dtype=np.uint32) >> np.uint32(9)).astype(np.float64)
    lo, hi = (extremes + 0.5) * 2.0 ** -23
    assert np.float32(lo) > 0 and np.float32(hi) < 1 and np.isfinite(-np.log(-np.log(np.float32(hi))))
    # another row, another draw, another seed: other numbers
    assert not np.array_equal(u[0], u[1])
    assert not np.array_equal(u, ref.uniforms(3, 4099, seed=2 ** 40 + 9, draw=6))
    assert not np.array_equal(u, ref.uniforms(3, 4099, seed=2 ** 40 + 10, draw=5))
    assert np.array_equal(u[1:2], ref.uniforms(1, 4099, seed=2 ** 40 + 9, draw=5, rows=[1]))


def tie_cases():
    """(name, row) of designed ties, V = 12"""
    V = 12
    two = np.where(np.arange(V) % 3 == 0, 2.0, -1.0)                       # 2.0 at 0, 3, 6, 9
    zeros = np.array([0.0, -0.0] * (V // 2))
    zeros[5], zeros[7] = 1.0, -1.0
    ninf = np.full(V, -np.inf)
    ninf[[2, 8]] = [0.5, -3.0]
    return [("all_equal", np.full(V, 1.5)), ("two_values", two), ("signed_zeros", zeros), ("minus_inf", ninf)]


@pytest.mark.parametrize("k", [1, 11, 12, 17])
def test_keep_mask_on_designed_ties(k):
    V = 12
    rows = dict(tie_cases())
    m = ref.keep_mask(np.stack(list(rows.values())), k)
    assert (m.sum(1) == min(k, V)).all()
    eq, two, zeros, ninf = m
    assert list(np.nonzero(eq)[0]) == list(range(min(k, V)))                # all equal: the k lowest indices
    if k == 1:
        assert list(np.nonzero(two)[0]) == [0] and list(np.nonzero(zeros)[0]) == [5] and list(np.nonzero(ninf)[0]) == [2]
    if k == 11:
        assert list(np.nonzero(~two)[0]) == [11]                            # the four 2.0, then -1.0 by index: the last one leaves
        assert list(np.nonzero(~zeros)[0]) == [7]                           # -0.0 == +0.0 > -1.0
        assert list(np.nonzero(~ninf)[0]) == [11]                           # -inf is a value like any other: the last index leaves
    m5 = ref.keep_mask(np.stack(list(rows.values())), 5)
    assert list(np.nonzero(m5[1])[0]) == [0, 1, 3, 6, 9]                    # four 2.0 and the first -1.0
    assert list(np.nonzero(m5[2])[0]) == [0, 1, 2, 3, 5]                    # 1.0 and the four first zeros of either sign
    assert list(np.nonzero(m5[3])[0]) == [0, 1, 2, 3, 8]                    # 0.5, -3.0 and the three first -inf


SEEDS = [77, 1, 2, 3, 12345, 2 ** 40 + 9]
LOGITS8 = np.array([2, 1, .5, 0, -.5, -1, -2, 1.5], dtype=np.float32)
CHI2_999_DF7 = 24.3                      # the 99.9 % point of chi-square at 7 degrees of freedom


def _chi2(tokens, p):
    n = len(tokens)
    counts = np.bincount(tokens, minlength=len(p)).astype(np.float64)
    return float(((counts - n * p) ** 2 / (n * p)).sum())


@pytest.mark.parametrize("seed", SEEDS)
def test_restated_draws_follow_the_softmax(seed):
    n, t = 16384, 0.7
    z = LOGITS8.astype(np.float64) / float(np.float32(t))
    p = np.exp(z - z.max())
    p /= p.sum()
    over_rows, _ = ref.sample(np.tile(LOGITS8, (n, 1)), t, None, seed, 0)
    # over draws, vectorised: row 0 of draw d is the block at counter (i / 4, 0, d_lo, d_hi)
    words = ref.philox4x32_10((np.arange(2, dtype=np.uint64)[None, :], 0, np.arange(n, dtype=np.uint64)[:, None], 0),
                              (seed & 0xffffffff, seed >> 32))
    u = ((np.stack(words, -1).reshape(n, 8) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    assert np.array_equal(u[5:6], ref.uniforms(1, 8, seed, 5))
    over_draws = np.argmax(z[None] - np.log(-np.log(u)), axis=1)
    for name, tokens in (("rows", over_rows), ("draws", over_draws)):
        x2 = _chi2(tokens, p)
        print(f"seed {seed} over {name}: chi-square {x2:.2f} (bound {CHI2_999_DF7})")
        assert x2 < CHI2_999_DF7, (name, x2)


def test_top_k_then_draw_stays_inside_the_kept_set():
    g = np.random.default_rng(0)
    logits = g.normal(0, 3, (32, 515)).astype(np.float32)
    tokens, gap = ref.sample(logits, 0.8, 50, 77, 3)
    keep = ref.keep_mask(logits, 50)
    assert keep[np.arange(32), tokens].all() and (gap >= 0).all()
    greedy, _ = ref.sample(logits, 0.0, 50, 77, 3)
    assert np.array_equal(greedy, logits.argmax(1))


# ---- 4. the host contract ------------------------------------------------------------------------------------------------------
def test_sampler_argument_errors_come_before_any_call():
    s = generate.Sampler(seed=5)
    logits = torch.zeros(2, 8)               # a CPU tensor: a call would raise RuntimeError, the argument checks come first
    for bad in (dict(temperature=-0.1), dict(temperature=float("nan")), dict(top_k=0), dict(top_k=-3), dict(top_k=2.5)):
        with pytest.raises(ValueError):
            s.sample(logits, **bad)
    with pytest.raises(ValueError):
        s.keep_mask(logits, 0)
    assert s.draws == 0 and s.seed == 5
    with pytest.raises(RuntimeError, match="no CPU path"):
        s.sample(logits)
    with pytest.raises(ValueError):
        s.sample(torch.zeros(8))
    assert s.draws == 0


def test_sampler_seed_comes_from_torchs_generator():
    torch.manual_seed(123)
    a = generate.Sampler()
    b = generate.Sampler()
    torch.manual_seed(123)
    c = generate.Sampler()
    assert a.seed == c.seed and a.seed != b.seed and a.draws == 0
    assert generate.Sampler(seed=2 ** 64 + 3).seed == 3
    assert generate._signed64(2 ** 63) == -2 ** 63 and generate._signed64(2 ** 64 - 1) == -1 and generate._signed64(7) == 7


def test_head_and_generate_argument_errors():
    head = generate.NextTokenHead(16, 40, vocab_size=33)
    assert list(head.state_dict()) == ["ln_f.weight", "lm_head.weight"] and head.lm_head.weight.shape == (40, 16)
    assert head.fused and head.vocab_size == 33 and generate.NextTokenHead(16, 40).vocab_size == 40
    with pytest.raises(ValueError):
        generate.NextTokenHead(16, 40, vocab_size=41)
    with pytest.raises(ValueError):
        head(torch.zeros(2, 3, 16), generate.Sampler(1), temperature=-1.0)
    with pytest.raises(RuntimeError):
        head.logits(torch.zeros(2, 3, 16))                                   # the kernels have no CPU path
    head.fused = False                                                       # the tensor-op restatement runs anywhere
    assert head.logits(torch.zeros(2, 3, 16)).shape == (2, 33) and head.logits(torch.zeros(2, 16)).shape == (2, 33)
    assert head(torch.randn(2, 3, 16), None, temperature=0.0, top_k=5).shape == (2,)
    with pytest.raises(ValueError):
        generate.last_logits(torch.zeros(2, 16), torch.zeros(40, 8))
    with pytest.raises(TypeError):
        generate.last_logits(torch.zeros(2, 16), torch.zeros(40, 16, dtype=torch.bfloat16))
    kw = dict(cos=torch.zeros(8, 4), sin=torch.zeros(8, 4))
    wte = torch.zeros(40, 16)
    with pytest.raises(ValueError, match="int64"):
        generate.generate(wte, [], head, [], torch.zeros(2, 3), 6, **kw)
    with pytest.raises(ValueError, match="exceed"):
        generate.generate(wte, [], head, [], torch.zeros(2, 3, dtype=torch.int64), 3, **kw)
    with pytest.raises(ValueError, match="rope cache"):
        generate.generate(wte, [], head, [], torch.zeros(2, 3, dtype=torch.int64), 10, **kw)
    with pytest.raises(ValueError, match="top_k"):
        generate.generate(wte, [], head, [], torch.zeros(2, 3, dtype=torch.int64), 6, top_k=0, **kw)
    with pytest.raises(ValueError, match="state caches"):
        generate.generate(wte, [], head, [None], torch.zeros(2, 3, dtype=torch.int64), 6, **kw)
