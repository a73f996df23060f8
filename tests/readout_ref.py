"""The attention readouts as numpy models (tests/test_readout_ad.py): Set2Set (GNNlib/src/layers/pool.jl:29-43) and GlobalAttentionPool
(pool.jl:7-12), their hand-written pullbacks, and the three exports of csrc/readout.hip by the formulas of include/gnnmp.h.

Every function computes in the dtype of its arguments: float64 arrays give the reference, float32 arrays the RESTATEMENT of the header's
formulas in the kernels' precision (numpy's own summation order, not the kernels').  The distance between the two conditions the test
operands and, where the fp32 summation bound does not cover a compounded error, sets the bar (weight_bar)."""
import functools

import numpy as np

f32, f64 = np.float32, np.float64
SEGS = (1, 2, 5, 63, 64, 65, 3, 700)                     # the batch: rows per graph; 700: many trips of the streaming loop and a remainder
SEGS_ABI = (1, 2, 5, 63, 0, 64, 65, 3, 700, 0)           # at the C ABI: an empty segment in the middle and one at the end
WIDTHS = (1, 2, 3, 4, 5, 8, 33, 64, 100, 130, 260)      # every lane-group width, every vector tail, a second feature tile (130, 260)
U32 = 2.0 ** -24
COND = 2e-6                                              # the float32 restatement of an export stays this close to float64, norm-wise
KINK = 1e-3                                              # relu pre-activations stay this far from 0


def gamma(n):
    return n * U32 / (1 - n * U32)


def rel(a, b):
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def worst(a, b):
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if b.size else 0.0


def ptr_of(segs):
    return np.concatenate([[0], np.cumsum(segs)]).astype(np.int64)


def indicator(segs, base=1):
    return np.repeat(np.arange(len(segs)), segs).astype(np.int64) + base


def cast(dtype, *arrs):
    return [None if a is None else np.asarray(a, dtype) for a in arrs]


def sigmoid(v):
    t = np.exp(-np.abs(v))
    return np.where(v >= 0, 1 / (1 + t), t / (1 + t)).astype(v.dtype)


def relu(v):
    return np.where(v < 0, v.dtype.type(0), v)


# ---- the three exports ---------------------------------------------------------------------------------------------------------------
def logits(x, rows, g, q, gate):
    return (x[rows] @ q[g])[:, None] if gate is None else gate[rows]


def pool(x, ptr, q=None, gate=None):
    """(r [G][D], stats [G][max(Dg,1)][2]) of gnnmp_segment_attn_pool_f32; an empty segment: r = 0, stats = (0, 0)"""
    dt, G, D = x.dtype, len(ptr) - 1, x.shape[1]
    Dg = 0 if gate is None else gate.shape[1]
    r, stats = np.zeros((G, D), dt), np.zeros((G, max(Dg, 1), 2), dt)
    for g in range(G):
        rows = slice(ptr[g], ptr[g + 1])
        if ptr[g + 1] == ptr[g]:
            continue
        s = logits(x, rows, g, q, gate)
        m = s.max(axis=0)
        p = np.exp(s - m)
        den = p.sum(axis=0, dtype=dt)
        r[g] = ((p / den) * x[rows]).sum(axis=0, dtype=dt)
        stats[g, :, 0], stats[g, :, 1] = m, den
    return r, stats


def pool_grad(dr, x, ptr, r, stats, q=None, gate=None, base=None):
    """(dq [G][D] | None, dx [N][D], dgate [N][Dg] | None) of gnnmp_segment_attn_pool_grad_f32"""
    dt, G = x.dtype, len(ptr) - 1
    dq = np.zeros_like(r) if gate is None else None
    dgate = None if gate is None else np.zeros_like(gate)
    dx = np.zeros_like(x) if base is None else np.array(base, dt)
    for g in range(G):
        rows = slice(ptr[g], ptr[g + 1])
        if ptr[g + 1] == ptr[g]:
            continue
        al = np.exp(logits(x, rows, g, q, gate) - stats[g, :, 0]) / stats[g, :, 1]
        c, t = dr[g] @ r[g], x[rows] @ dr[g]
        dx[rows] = dx[rows] + al * dr[g]
        if gate is None:
            ds = al[:, 0] * (t - c)
            dq[g] = ds @ x[rows]
            dx[rows] = dx[rows] + ds[:, None] * q[g]
        elif gate.shape[1] == 1:
            dgate[rows, 0] = al[:, 0] * (t - c)
        else:
            dgate[rows] = (al * dr[g]) * (x[rows] - r[g])
    return dq, dx, dgate


def gates(gx, gh, b, n):
    a = gx + gh + (0 if b is None else b)
    return sigmoid(a[:, :n]), sigmoid(a[:, n:2 * n]), np.tanh(a[:, 2 * n:3 * n]), sigmoid(a[:, 3 * n:])


def lstm(gx, gh, b, c):
    """(h', c') of gnnmp_lstm_pointwise_f32: gates input, forget, cell, output"""
    i, f, g, o = gates(gx, gh, b, c.shape[1])
    cn = f * c + i * g
    return o * np.tanh(cn), cn


def lstm_grad(gx, gh, b, c, dh, dcn=None):
    """(da [N][4D], dc [N][D]) of gnnmp_lstm_pointwise_grad_f32"""
    i, f, g, o = gates(gx, gh, b, c.shape[1])
    T = np.tanh(f * c + i * g)
    dct = (0 if dcn is None else dcn) + dh * o * (1 - T * T)
    da = np.concatenate([dct * g * (i * (1 - i)), dct * c * (f * (1 - f)), dct * i * (1 - g * g), dh * T * (o * (1 - o))], axis=1)
    return da, dct * f


# ---- Set2Set ---------------------------------------------------------------------------------------------------------------------------
def set2set(x, ptr, Wi, Wh, b, iters):
    """(vcat(q, r) [G][2n], trace)"""
    dt, G, n = x.dtype, len(ptr) - 1, x.shape[1]
    q, r, c = np.zeros((G, n), dt), np.zeros((G, n), dt), np.zeros((G, n), dt)
    trace = []
    for _ in range(iters):
        qs = np.concatenate([q, r], axis=1)
        gx, gh = qs @ Wi.T, q @ Wh.T
        hn, cn = lstm(gx, gh, b, c)
        rn, stats = pool(x, ptr, q=hn)
        trace.append(dict(qs=qs, h=q, gx=gx, gh=gh, c=c, q=hn, r=rn, stats=stats))
        q, r, c = hn, rn, cn
    return np.concatenate([q, r], axis=1), trace


def set2set_grad(x, ptr, Wi, Wh, b, iters, dout):
    """dict(y, dx, dWi, dWh, db) and, for the summation bound, the magnitudes mWi, mWh, mb = Σ|terms| of the three stacked folds and n, the
    longest fold on the path: the longest segment (r and dq), the iters * G stacked rows, or the 4 n_in terms of da Wi"""
    n = x.shape[1]
    y, trace = set2set(x, ptr, Wi, Wh, b, iters)
    dh, dr = dout[:, :n], dout[:, n:]
    dcn, dx, das = None, None, []
    for k in range(iters - 1, -1, -1):
        tr = trace[k]
        dq, dx, _ = pool_grad(dr, x, ptr, tr["r"], tr["stats"], q=tr["q"], base=dx)
        da, dcn = lstm_grad(tr["gx"], tr["gh"], b, tr["c"], dh + dq, dcn)
        das.append(da)
        dqs = da @ Wi
        dh, dr = dqs[:, :n] + da @ Wh, dqs[:, n:]
    DA = np.concatenate(das[::-1])
    QS, H = np.concatenate([tr["qs"] for tr in trace]), np.concatenate([tr["h"] for tr in trace])
    return dict(y=y, dx=dx, dWi=DA.T @ QS, dWh=DA.T @ H, db=DA.sum(axis=0), mWi=np.abs(DA).T @ np.abs(QS), mWh=np.abs(DA).T @ np.abs(H),
                mb=np.abs(DA).sum(axis=0), n=int(max(np.diff(ptr).max(), DA.shape[0], 4 * n)))


# ---- GlobalAttentionPool -----------------------------------------------------------------------------------------------------------------
def chain_forward(h, chain):
    """(output, [(input, pre-activation)]) of a list of (W, b | None, None | 'relu')"""
    trace = []
    for W, b, act in chain:
        pre = h @ W.T + (0 if b is None else b)
        trace.append((h, pre))
        h = relu(pre) if act == "relu" else pre
    return h, trace


def chain_backward(d, chain, trace):
    """(d input, [(dW, db, |terms| of dW, |terms| of db)])"""
    grads = []
    for (W, b, act), (inp, pre) in zip(reversed(chain), reversed(trace)):
        if act == "relu":
            d = d * (pre > 0)
        grads.append((d.T @ inp, d.sum(axis=0), np.abs(d).T @ np.abs(inp), np.abs(d).sum(axis=0)))
        d = d @ W
    return d, grads[::-1]


def gap(x, ptr, fgate, ffeat):
    gate, tg = chain_forward(x, fgate)
    feats, tf = chain_forward(x, ffeat) if ffeat else (x, [])
    r, stats = pool(feats, ptr, gate=gate)
    return r, (gate, tg, feats, tf, stats)


def gap_grad(x, ptr, fgate, ffeat, dr):
    """dict(y, dx, fgate = [(dW, db, mW, mb)], ffeat = [...], pres = the relu pre-activations)"""
    r, (gate, tg, feats, tf, stats) = gap(x, ptr, fgate, ffeat)
    _, dfeats, dgate = pool_grad(dr, feats, ptr, r, stats, gate=gate)
    dx, gg = chain_backward(dgate, fgate, tg)
    gf = []
    if ffeat:
        dxf, gf = chain_backward(dfeats, ffeat, tf)
        dx = dx + dxf
    else:
        dx = dx + dfeats
    pres = [pre for (_, _, act), (_, pre) in zip(list(fgate) + list(ffeat or []), tg + tf) if act == "relu"]
    return dict(y=r, dx=dx, fgate=gg, ffeat=gf, pres=pres)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool_case(D, Dg, seed=0, segs=SEGS_ABI):
    """float32 operands of one export case: (x, ptr, q | None, gate | None, dr, base); logits of order 1"""
    rng = np.random.default_rng([11, D, Dg, seed])
    ptr = ptr_of(segs)
    N, G = int(ptr[-1]), len(segs)
    x = rng.standard_normal((N, D)).astype(f32)
    q = (rng.standard_normal((G, D)) / np.sqrt(D)).astype(f32) if Dg == 0 else None
    gate = rng.standard_normal((N, Dg)).astype(f32) if Dg else None
    dr = rng.standard_normal((G, D)).astype(f32)
    base = rng.standard_normal((N, D)).astype(f32)
    return x, ptr, q, gate, dr, base


@functools.lru_cache(maxsize=None)
def pool_ref(D, Dg, seed=0, dtype="float64", segs=SEGS_ABI):
    """dict(r, stats, dq, dx, dgate, dx_base) of the case in `dtype`"""
    x, ptr, q, gate, dr, base = pool_case(D, Dg, seed, segs)
    x, q, gate, dr, base = cast(np.dtype(dtype), x, q, gate, dr, base)
    r, stats = pool(x, ptr, q, gate)
    dq, dx, dgate = pool_grad(dr, x, ptr, r, stats, q, gate)
    return dict(r=r, stats=stats, dq=dq, dx=dx, dgate=dgate, dx_base=pool_grad(dr, x, ptr, r, stats, q, gate, base)[1])


def pool_condition(D, Dg, seed=0):
    """the largest norm-wise distance of the float32 restatement from float64 over the case's outputs"""
    a, b = pool_ref(D, Dg, seed, "float32"), pool_ref(D, Dg, seed)
    return max(rel(a[k], b[k]) for k in a if a[k] is not None)


@functools.lru_cache(maxsize=None)
def lstm_case(N, D, seed=0):
    rng = np.random.default_rng([12, N, D, seed])
    mk = lambda *s: rng.standard_normal(s).astype(f32)      # noqa: E731
    return mk(N, 4 * D), mk(N, 4 * D), mk(4 * D), mk(N, D), mk(N, D), mk(N, D)      # gx, gh, b, c, dh, dcn


def glorot(rng, out, cin):
    return (rng.uniform(-1, 1, (out, cin)) * np.sqrt(6.0 / (out + cin))).astype(f32)


@functools.lru_cache(maxsize=None)
def set2set_case(n, seed=0, segs=SEGS):
    """(x, ptr, Wi, Wh, b, dout), float32"""
    rng = np.random.default_rng([13, n, seed])
    ptr = ptr_of(segs)
    x = rng.standard_normal((int(ptr[-1]), n)).astype(f32)
    return x, ptr, glorot(rng, 4 * n, 2 * n), glorot(rng, 4 * n, n), (0.1 * rng.standard_normal(4 * n)).astype(f32), \
        rng.standard_normal((len(segs), 2 * n)).astype(f32)


@functools.lru_cache(maxsize=None)
def set2set_ref(n, iters, seed=0, dtype="float64", segs=SEGS):
    x, ptr, Wi, Wh, b, dout = set2set_case(n, seed, segs)
    x, Wi, Wh, b, dout = cast(np.dtype(dtype), x, Wi, Wh, b, dout)
    return set2set_grad(x, ptr, Wi, Wh, b, iters, dout)


GAP_VARIANTS = [(Dg, ffeat) for Dg in ("one", "all") for ffeat in (True, False)]      # gate channels: 1 or D'; with and without ffeat


def _gap_build(D, Dg, with_ffeat, seed, segs):
    rng = np.random.default_rng([14, D, Dg == "all", with_ffeat, seed])
    ptr = ptr_of(segs)
    x = rng.standard_normal((int(ptr[-1]), D)).astype(f32)
    Df = D + 1 if with_ffeat else D
    hid = 6
    mkb = lambda k: (0.1 * rng.standard_normal(k)).astype(f32)      # noqa: E731
    fgate = [(glorot(rng, hid, D), mkb(hid), "relu"), (glorot(rng, 1 if Dg == "one" else Df, hid), mkb(1 if Dg == "one" else Df), None)]
    ffeat = [(glorot(rng, Df, D), mkb(Df), "relu")] if with_ffeat else None
    dr = rng.standard_normal((len(segs), Df)).astype(f32)
    firsts = [np.asarray(c[0][0], f64) for c in (fgate, ffeat) if c], [np.asarray(c[0][1], f64) for c in (fgate, ffeat) if c]
    for _ in range(100):      # the relu layers are the first of each chain: a row with a pre-activation near 0 is drawn again
        near = np.zeros(len(x), bool)
        for W, b in zip(*firsts):
            near |= (np.abs(np.asarray(x, f64) @ W.T + b) < 4 * KINK).any(axis=1)
        if not near.any():
            break
        x[near] = rng.standard_normal((int(near.sum()), D)).astype(f32)
    return x, ptr, fgate, ffeat, dr


def chain64(chain):
    return None if chain is None else [(np.asarray(W, f64), None if b is None else np.asarray(b, f64), act) for W, b, act in chain]


@functools.lru_cache(maxsize=None)
def gap_case(D, Dg, with_ffeat, segs=SEGS, margin=KINK):
    """(x, ptr, fgate, ffeat, dr) float32 with every relu pre-activation at least `margin` from 0 (the builder redraws the rows of x that
    come near a kink; this is the check): the first seed that meets it"""
    for seed in range(20):
        x, ptr, fgate, ffeat, dr = case = _gap_build(D, Dg, with_ffeat, seed, segs)
        ref = gap_grad(np.asarray(x, f64), ptr, chain64(fgate), chain64(ffeat), np.asarray(dr, f64))
        if min(float(np.abs(p).min()) for p in ref["pres"]) >= margin:
            return case
    raise AssertionError("no seed keeps the relu pre-activations away from 0")


@functools.lru_cache(maxsize=None)
def gap_ref(D, Dg, with_ffeat, dtype="float64", segs=SEGS):
    x, ptr, fgate, ffeat, dr = gap_case(D, Dg, with_ffeat, segs)
    dt = np.dtype(dtype)
    ch = lambda c: None if c is None else [(np.asarray(W, dt), np.asarray(b, dt), act) for W, b, act in c]      # noqa: E731
    return gap_grad(np.asarray(x, dt), ptr, ch(fgate), ch(ffeat), np.asarray(dr, dt))


# ---- the bar of the weight gradients -----------------------------------------------------------------------------------------------------
def bound_used(got, ref, mag, n):
    """the largest |got - ref| / (γ_n Σ|terms|), element-wise"""
    got, ref, mag = np.asarray(got, f64), np.asarray(ref, f64), np.asarray(mag, f64)
    return float((np.abs(got - ref) / np.maximum(gamma(n) * mag, 1e-300)).max())


def weight_bar(rest, ref, mag, n):
    """How a weight gradient is judged.  ('sum', γ_n Σ|terms|) when the float32 restatement of the reference, on the CPU, is itself inside
    the fp32 summation bound of the last fold; otherwise the compounded error of the path is not a summation error of that fold and the
    bar is ('restatement', 4 × the restatement's own distance from float64 — norm-wise and element-wise against the array scale; the
    factor 4 for another fold order)."""
    if bound_used(rest, ref, mag, n) <= 1.0:
        return "sum", gamma(n) * np.asarray(mag, f64)
    return "restatement", 4.0 * max(rel(rest, ref), worst(rest, ref))
