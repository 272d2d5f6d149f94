"""CPU-side checks of the multi-token continuation of the second-order decode state cache (fastmax_hip_p2_extend,
FastmaxDecodeState.extend, prefill(chunk=...)): the entry points are exported and declared, the workspace size follows the
documented rules, and every rejected argument comes back as its error code before anything is launched (host pointers stand
in for device buffers: a rejected call never touches them)."""
import ctypes
import os
import re

import pytest

from fastmax_experiments_amd._lib import Problem, PATH_AUTO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["fastmax_hip_p2_extend_workspace", "fastmax_hip_p2_extend"]
E_BAD_P, E_BAD_SHAPE, E_BAD_DTYPE, E_WORKSPACE, E_NULL = -1, -2, -3, -4, -6


@pytest.fixture(scope="module")
def lib():
    from fastmax_experiments_amd import _lib, build
    build.build()
    return _lib.lib()


def test_symbols_exported_and_declared(lib):
    from fastmax_experiments_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fastmax_hip.h")).read()
    declared = set(re.findall(r"\b(fastmax_hip_[a-z0-9_]+)\s*\(", hdr))
    for s in NEW:
        assert s in declared and s in _lib.SYMBOLS and hasattr(lib, s), s
    assert lib.fastmax_hip_abi_version() == 9
    assert "#define FASTMAX_ABI_VERSION 9" in hdr


def test_workspace_bytes(lib):
    f = lib.fastmax_hip_p2_extend_workspace
    # what p2_decode_state_bytes rejects, T <= 0 and query heads that do not divide into the KV heads
    for B, H, Hkv, T, D in ((0, 4, 4, 8, 64), (1, 4, 0, 8, 64), (1, 4, 4, 8, 0), (1, 4, 4, 8, 129), (-1, 4, 4, 8, 64),
                            (1, 4, -2, 8, 64), (1, 4, 4, 8, -8), (1, 4, 4, 0, 64), (1, 4, 4, -3, 64), (1, 4, 3, 8, 64),
                            (1, 6, 4, 8, 64), (1, 0, 4, 8, 64)):
        assert f(B, H, Hkv, T, D) == 0, (B, H, Hkv, T, D)
        if B > 0 and Hkv > 0 and 0 < D <= 128:
            assert lib.fastmax_hip_p2_decode_state_bytes(B, Hkv, D) > 0
        elif T > 0 and H > 0 and Hkv > 0 and H % Hkv == 0:
            assert lib.fastmax_hip_p2_decode_state_bytes(B, Hkv, D) == 0
    for B, H, Hkv, D in ((1, 32, 32, 64), (1, 32, 4, 64), (8, 32, 32, 64), (1, 2, 2, 128), (1, 8, 1, 33), (2, 3, 3, 1)):
        prev = 0
        for T in list(range(1, 300)) + [511, 512, 513, 1024, 4096, 4097]:
            w = f(B, H, Hkv, T, D)
            assert w > 0 and w % 16 == 0, (B, H, Hkv, T, D)
            assert w >= prev, (B, H, Hkv, T, D, w, prev)
            # at least the chunk's fp32 numerator and denominator
            assert w >= 4 * B * H * T * (D + 1)
            prev = w


def _bufs():
    keep = [ctypes.create_string_buffer(4096) for _ in range(6)]
    ptrs = [ctypes.cast(b, ctypes.c_void_p) for b in keep]
    st = (ctypes.c_int64 * 3)(64 * 16 * 4, 64 * 16, 64)
    return keep, ptrs, st


def test_extend_rejects_bad_arguments(lib):
    keep, (q, k, v, state, o, ws), st = _bufs()
    ext = lib.fastmax_hip_p2_extend
    big = 1 << 40                       # a size, not a buffer: a rejected call never touches the workspace

    def prob(B=1, H=4, Nq=16, Nk=16, D=64, dt=1, odt=1, p=2, causal=1):
        return Problem(B, H, Nq, Nk, D, dt, odt, p, causal, 0.125, 1 / 128, 0.0, PATH_AUTO)

    def call(pr, Hkv=2, q=q, k=k, v=v, state=state, o=o, qs=st, ks=st, vs=st, ws=ws, nbytes=big):
        return ext(ctypes.byref(pr) if pr is not None else None, Hkv, q, qs, k, ks, v, vs,
                   ctypes.cast(state, ctypes.c_void_p), o, ws, nbytes, None)

    assert call(None) == E_NULL
    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(state=None), dict(o=None), dict(qs=None), dict(ks=None),
               dict(vs=None)):
        assert call(prob(), **kw) == E_NULL, kw
    for kw in (dict(p=1), dict(p=3), dict(p=0), dict(causal=0)):
        assert call(prob(**kw)) == E_BAD_P, kw
    for kw in (dict(Nq=16, Nk=17), dict(Nq=8, Nk=16), dict(Nq=0, Nk=0), dict(D=0), dict(D=129), dict(B=0), dict(H=0)):
        assert call(prob(**kw)) == E_BAD_SHAPE, kw
    assert call(prob(H=4), Hkv=3) == E_BAD_SHAPE
    assert call(prob(H=6), Hkv=4) == E_BAD_SHAPE
    assert call(prob(), Hkv=0) == E_BAD_SHAPE
    for kw in (dict(dt=3), dict(dt=-1), dict(odt=7), dict(odt=-2)):
        assert call(prob(**kw)) == E_BAD_DTYPE, kw
    need = lib.fastmax_hip_p2_extend_workspace(1, 4, 2, 16, 64)
    assert need > 0
    assert call(prob(), ws=None) == E_WORKSPACE
    assert call(prob(), nbytes=need - 1) == E_WORKSPACE
    assert call(prob(), nbytes=0) == E_WORKSPACE


def test_python_rejections():
    from fastmax_experiments_amd.decode import FastmaxDecodeState
    import torch
    x = torch.zeros(1, 4, 3, 64)
    st1 = FastmaxDecodeState(1, 4, 64, "cpu", p=1)
    with pytest.raises(NotImplementedError, match="p=2"):
        st1.extend(x, x, x)
    st2 = FastmaxDecodeState(1, 4, 64, "cpu", p=2, n_query_groups=2)
    for c in (0, -4):
        with pytest.raises(ValueError):
            st2.prefill(x, x[:, :2], x[:, :2], chunk=c)
        with pytest.raises(ValueError):
            st1.prefill(x, x, x, chunk=c)
    # the shape check of step / prefill: k, v carry the KV heads
    with pytest.raises(ValueError):
        st2.extend(x, x, x)
    with pytest.raises(ValueError):
        st2.extend(x[:, :, :0], x[:, :2, :0], x[:, :2, :0])
    assert st2.count == 0
