"""float64 numpy restatements of the mixture-of-experts MLP (lit_gpt/model.py:644-674) around its expert MLPs: the routing
(selection with its tie rule, the softmax over the selected values, the stable dispatch arrays), the combine with the
reference's rounding points, and ``exact=True`` forms without any rounding for the gradient checks.  Built on block_ref.py.
Shared by test_moe_cpu.py (which proves the restatements on the fixtures) and test_moe_gpu.py."""
import numpy as np

from block_ref import MANT, act_ref, act_ref32, round_to


def select(router, k):
    """(M, k) expert ids in ASCENDING id: the k largest of each row, ties to the lowest index, NaN above every number"""
    r = np.asarray(router, np.float64)
    with np.errstate(invalid="ignore"):
        key = np.where(np.isnan(r), np.inf, np.minimum(r, np.finfo(np.float64).max))       # NaN above +inf
    order = np.argsort(-key, axis=1, kind="stable")            # stable: equal keys keep ascending index
    return np.sort(order[:, :k], axis=1).astype(np.int32)


def route(router, k, dt, exact=False):
    """-> dict(expert, prob32, prob, offsets, row_of, slot_of).  prob32 is the float64 softmax (the tests bound the kernel's
    float32 against it), prob its rounding to dt through float32 (left unrounded with exact)"""
    r = np.asarray(router, np.float64)
    M, E = r.shape
    expert = select(r, k)
    v = np.take_along_axis(r, expert, axis=1)
    with np.errstate(invalid="ignore"):
        ex = np.exp(v - v.max(axis=1, keepdims=True))
        prob32 = ex / ex.sum(axis=1, keepdims=True)
    prob = prob32 if exact else round_to(round_to(prob32, "f32"), dt)
    # stable counting sort of the (token, j) pairs by expert: expert e's tokens ascending, as torch.where yields them
    flat = expert.reshape(-1)
    order = np.argsort(flat, kind="stable")
    counts = np.bincount(flat, minlength=E)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    row_of = (order // k).astype(np.int32)
    slot_of = np.empty(M * k, np.int32)
    slot_of[order] = np.arange(M * k, dtype=np.int32)
    return dict(expert=expert, prob32=prob32, prob=prob, offsets=offsets, row_of=row_of, slot_of=slot_of.reshape(M, k))


def combine(ys, prob, slot_of, dt, exact=False):
    """y[t] = 0; j ascending: y[t] = round(y[t] + round(prob[t, j] ys[slot_of[t, j]]))"""
    rnd = (lambda a, d: a) if exact else round_to
    ys, prob = np.asarray(ys, np.float64), np.asarray(prob, np.float64)
    y = np.zeros((slot_of.shape[0], ys.shape[1]))
    for j in range(slot_of.shape[1]):
        y = rnd(y + rnd(prob[:, j, None] * ys[slot_of[:, j]], dt), dt)
    return y


def combine_backward(dy, ys, prob, slot_of):
    """exact: -> (dys, dprob)"""
    dy, ys, prob = (np.asarray(a, np.float64) for a in (dy, ys, prob))
    dys, dprob = np.zeros_like(ys), np.zeros_like(prob)
    for j in range(slot_of.shape[1]):
        dys[slot_of[:, j]] = prob[:, j, None] * dy
        dprob[:, j] = (dy * ys[slot_of[:, j]]).sum(axis=1)
    return dys, dprob


def gather_backward(dxs, slot_of):
    dxs = np.asarray(dxs, np.float64)
    return sum(dxs[slot_of[:, j]] for j in range(slot_of.shape[1]))


def route_backward(dprob, prob, expert, E):
    """exact: the softmax's backward over the selected values, scattered into a zero (M, E)"""
    g, p = np.asarray(dprob, np.float64), np.asarray(prob, np.float64)
    d = p * (g - (p * g).sum(axis=1, keepdims=True))
    out = np.zeros((g.shape[0], E))
    np.put_along_axis(out, expert.astype(np.int64), d, axis=1)
    return out


def mlp(x, w1, w2, wp, dt, exact=False):
    """LLaMAMLP (model.py:629-633): proj(silu(fc_1 x) * fc_2 x), every tensor op rounded to dt"""
    rnd = (lambda a, d: a) if exact else round_to
    x, w1, w2, wp = (np.asarray(a, np.float64) for a in (x, w1, w2, wp))
    a, b = rnd(x @ w1.T, dt), rnd(x @ w2.T, dt)
    act = act_ref(a, "silu") if exact else round_to(act_ref32(a, "silu"), dt)
    return rnd(rnd(act * b, dt) @ wp.T, dt)


def moe_forward(x, router, experts, k, dt, exact=False):
    """the whole layer over the gate output `router` it saw; experts: [(fc_1, fc_2, proj) weights]"""
    x = np.asarray(x, np.float64)
    r = route(router, k, dt, exact)
    xs = x[r["row_of"]]
    ys = np.zeros_like(xs)
    for e, (w1, w2, wp) in enumerate(experts):
        a, b = r["offsets"][e], r["offsets"][e + 1]
        if b > a:
            ys[a:b] = mlp(xs[a:b], w1, w2, wp, dt, exact)
    return combine(ys, r["prob"], r["slot_of"], dt, exact), r, ys


def moe_backward(x, gate_w, experts, k, gy, select_from=None):
    """exact gradients of the whole layer at a fixed selection (the selection is piecewise constant): -> (dx, dgate, [(d fc_1,
    d fc_2, d proj)]).  The selection is that of `select_from` (the gate output a run saw) or of the exact router x gate^T;
    the probabilities are always the exact router's"""
    x, gate_w, gy = (np.asarray(a, np.float64) for a in (x, gate_w, gy))
    E = gate_w.shape[0]
    router = x @ gate_w.T
    r = route(router if select_from is None else select_from, k, "f32", exact=True)
    if select_from is not None:
        v = np.take_along_axis(router, r["expert"], axis=1)
        ex = np.exp(v - v.max(axis=1, keepdims=True))
        r["prob"] = r["prob32"] = ex / ex.sum(axis=1, keepdims=True)
    xs = x[r["row_of"]]
    ys, dxs, dws = np.zeros_like(xs), np.zeros_like(xs), []
    for e, (w1, w2, wp) in enumerate(experts):
        lo, hi = r["offsets"][e], r["offsets"][e + 1]
        w1, w2, wp = (np.asarray(w, np.float64) for w in (w1, w2, wp))
        a, b = xs[lo:hi] @ w1.T, xs[lo:hi] @ w2.T
        ys[lo:hi] = (act_ref(a, "silu") * b) @ wp.T
        dws.append((a, b, w1, w2, wp, lo, hi))
    dys, dprob = combine_backward(gy, ys, r["prob"], r["slot_of"])
    grads = []
    for a, b, w1, w2, wp, lo, hi in dws:
        sig = 1.0 / (1.0 + np.exp(-a))
        act = a * sig
        g = act * b
        dg = dys[lo:hi] @ wp
        da, db = dg * b * (sig * (1.0 + a * (1.0 - sig))), dg * act
        dxs[lo:hi] = da @ w1 + db @ w2
        grads.append((da.T @ xs[lo:hi], db.T @ xs[lo:hi], dys[lo:hi].T @ g))
    drouter = route_backward(dprob, r["prob"], r["expert"], E)
    dx = gather_backward(dxs, r["slot_of"]) + drouter @ gate_w
    return dx, drouter.T @ x, grads


def rel_to_max(got, exact):
    """max |got - exact| / max |exact|: the backward tests' measure"""
    got, exact = np.asarray(got, np.float64), np.asarray(exact, np.float64)
    return float(np.abs(got - exact).max() / np.abs(exact).max())


def eps(dt):
    return 2.0 ** -MANT[dt]
