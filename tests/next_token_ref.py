"""numpy restatement of the next-token head's sampler (include/fastmax_hip_next_token.h), float64 unless stated: Philox-4x32-10,
the uniforms, the keep mask of the exact top-k, the scores and the token.  Shared by test_next_token_cpu.py and
test_next_token_gpu.py; nothing here touches the library."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcastable), key: two ints -> four uint32 arrays"""
    c = [np.asarray(x, dtype=np.uint64) & MASK32 for x in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)                # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK32, p1 >> np.uint64(32), p1 & MASK32
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [x.astype(np.uint32) for x in c]


def uniforms(B, V, seed, draw, rows=None):
    """u[b, i] = ((word >> 9) + 0.5) 2^-23, word i % 4 of the block at counter (i / 4, b, draw_lo, draw_hi), key (seed_lo, seed_hi)"""
    seed, draw = int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1)
    nq = (V + 3) // 4
    rows = np.arange(B, dtype=np.uint64) if rows is None else np.asarray(rows, dtype=np.uint64)
    words = philox4x32_10((np.arange(nq, dtype=np.uint64)[None, :], rows[:, None], draw & MASK32, draw >> 32),
                          (seed & MASK32, seed >> 32))
    w = np.stack(words, axis=-1).reshape(len(rows), nq * 4)[:, :V]
    return ((w >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def order_key(x):
    """float32 -> uint32, larger value <=> larger key; -0.0 shares +0.0's key"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def keep_mask(logits, top_k):
    """bool (B, V): exactly top_k per row -- above the k-th largest value, and of those equal to it the lowest indices"""
    logits = np.asarray(logits, dtype=np.float32)
    B, V = logits.shape
    if top_k is None or top_k >= V:
        return np.ones((B, V), dtype=bool)
    keys = order_key(logits)
    out = np.zeros((B, V), dtype=bool)
    for b in range(B):
        t = np.sort(keys[b])[V - top_k]
        above = keys[b] > t
        ties = np.nonzero(keys[b] == t)[0][:top_k - int(above.sum())]
        out[b] = above
        out[b, ties] = True
    return out


def scores(logits, temperature, seed, draw, rows=None):
    """logit / temperature - log(-log u) in float64 (temperature as the float32 the library receives); the logits themselves
    at temperature 0"""
    logits = np.asarray(logits, dtype=np.float32).astype(np.float64)
    if temperature == 0:
        return logits
    u = uniforms(logits.shape[0], logits.shape[1], seed, draw, rows)
    with np.errstate(divide="ignore"):
        return logits / float(np.float32(temperature)) - np.log(-np.log(u))


def sample(logits, temperature, top_k, seed, draw, rows=None):
    """-> (tokens (B,), gap (B,)): the kept entry with the best score (lowest index on ties) and the float64 distance to the
    runner-up among the kept entries (inf when only one is kept)"""
    s = np.where(keep_mask(logits, top_k), scores(logits, temperature, seed, draw, rows), -np.inf)
    tokens = np.argmax(s, axis=1)
    if s.shape[1] == 1:
        return tokens, np.full(s.shape[0], np.inf)
    top2 = np.partition(s, s.shape[1] - 2, axis=1)[:, -2:]
    with np.errstate(invalid="ignore"):
        gap = top2[:, 1] - top2[:, 0]
    return tokens, np.where(np.isnan(gap), 0.0, gap)
