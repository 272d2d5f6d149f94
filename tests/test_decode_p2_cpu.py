"""CPU-side checks of the second-order decode state cache (csrc/fastmax_decode_p2.hip, decode.py): the three entry points are
exported and declared, the state size follows the documented rules, and every rejected argument comes back as its error
code before anything is launched (host pointers stand in for device buffers: a rejected call never touches them)."""
import ctypes
import os
import re

import pytest

from fastmax_experiments_amd._lib import Problem, PATH_AUTO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P2 = ["fastmax_hip_p2_decode_state_bytes", "fastmax_hip_p2_prefill_state", "fastmax_hip_p2_decode_step"]
E_BAD_P, E_BAD_SHAPE, E_BAD_DTYPE, E_NULL = -1, -2, -3, -6


@pytest.fixture(scope="module")
def lib():
    from fastmax_experiments_amd import _lib, build
    build.build()
    return _lib.lib()


def test_symbols_exported_and_declared(lib):
    from fastmax_experiments_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fastmax_hip.h")).read()
    declared = set(re.findall(r"\b(fastmax_hip_[a-z0-9_]+)\s*\(", hdr))
    for s in P2:
        assert s in declared and s in _lib.SYMBOLS and hasattr(lib, s), s
    assert lib.fastmax_hip_abi_version() == 9


def test_state_bytes(lib):
    f = lib.fastmax_hip_p2_decode_state_bytes
    for B, Hkv, D in ((0, 4, 64), (1, 0, 64), (1, 4, 0), (1, 4, 129), (-1, 4, 64), (1, -2, 64), (1, 4, -8)):
        assert f(B, Hkv, D) == 0, (B, Hkv, D)
    for D in (1, 40, 64, 128):
        base = f(1, 1, D)
        assert base > 0 and base % 16 == 0
        # at least the (D+1)(D+2)/2 pair rows of D+1 floats
        assert base >= 4 * (D + 1) * (D + 2) // 2 * (D + 1)
        assert f(2, 1, D) > base and f(1, 3, D) > base and f(2, 3, D) > f(1, 3, D)
        assert f(2, 3, D) == 6 * base
    # sized per KV head: the query heads of a group share one record (the argument IS the KV head count)
    assert f(2, 4, 64) == 4 * f(2, 1, 64)
    assert f(1, 32, 64) < 32 * 0.6e6 * 1.2 and f(1, 1, 128) < 4.4e6 * 1.1


def _bufs():
    keep = [ctypes.create_string_buffer(4096) for _ in range(5)]
    ptrs = [ctypes.cast(b, ctypes.c_void_p) for b in keep]
    st = (ctypes.c_int64 * 3)(64 * 16, 64 * 16, 64)
    return keep, ptrs, st


def test_step_rejects_bad_arguments(lib):
    keep, (q, k, v, state, o), st = _bufs()
    step = lib.fastmax_hip_p2_decode_step

    def call(q=q, k=k, v=v, state=state, o=o, qs=st, B=1, H=4, Hkv=2, D=64, dt=1, odt=1):
        return step(q, qs, k, st, v, st, ctypes.cast(state, ctypes.c_void_p), o, B, H, Hkv, D, dt, odt, 0.125, None)

    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(state=None), dict(o=None), dict(qs=None)):
        assert call(**kw) == E_NULL, kw
    for kw in (dict(H=4, Hkv=3), dict(H=6, Hkv=4), dict(D=129), dict(D=0), dict(B=0), dict(H=0), dict(Hkv=0)):
        assert call(**kw) == E_BAD_SHAPE, kw
    for kw in (dict(dt=3), dict(dt=-1), dict(odt=7)):
        assert call(**kw) == E_BAD_DTYPE, kw


def test_prefill_rejects_bad_arguments(lib):
    keep, (q, k, v, state, o), st = _bufs()
    pre = lib.fastmax_hip_p2_prefill_state

    def call(prob, k=k, v=v, state=state):
        return pre(ctypes.byref(prob) if prob is not None else None, k, st, v, st, ctypes.cast(state, ctypes.c_void_p), None)

    def prob(B=1, H=2, N=16, D=64, dt=1, p=2, causal=1):
        return Problem(B, H, N, N, D, dt, dt, p, causal, 0.125, 1 / 128, 0.0, PATH_AUTO)

    assert call(None) == E_NULL
    assert call(prob(), k=None) == E_NULL
    assert call(prob(), v=None) == E_NULL
    assert call(prob(), state=None) == E_NULL
    assert call(prob(p=1)) == E_BAD_P
    assert call(prob(p=3)) == E_BAD_P
    assert call(prob(D=129)) == E_BAD_SHAPE
    assert call(prob(N=0)) == E_BAD_SHAPE
    assert call(prob(B=0)) == E_BAD_SHAPE
    assert call(prob(dt=5)) == E_BAD_DTYPE


def test_decode_state_rejects_bad_p():
    from fastmax_experiments_amd.decode import FastmaxDecodeState
    for p in (0, 3):
        with pytest.raises(ValueError):
            FastmaxDecodeState(1, 4, 64, "cpu", p=p)
    with pytest.raises(ValueError):
        FastmaxDecodeState(1, 4, 64, "cpu", p=1, n_query_groups=2)
    with pytest.raises(ValueError):
        FastmaxDecodeState(1, 4, 64, "cpu", p=2, n_query_groups=3)
