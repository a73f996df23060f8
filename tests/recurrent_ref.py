"""A torch model of the graph-convolutional recurrent cells (tests/test_recurrent_layers.py): GConvGRUCell, GConvLSTMCell and DCGRUCell
term by term as GraphNeuralNetworks/src/layers/temporalconv.jl:237-254, :416-437 and :564-575 write them, and their scan over time
(:121-135).  It stands on the hop of tests/poly_conv_ref.py (restated in torch so that autograd sees it; a test pins the two together),
works in the dtype of its operands — the same text is the float32 restatement the input conditions use — and takes its gradients from
torch autograd.  Also the float64 numpy restatement of the gate kernels' header formulas (include/gnnmp.h).
Edge k: s[k] -> t[k], 0-based."""
import numpy as np
import torch

import poly_conv_ref as R

f32, f64 = np.float32, np.float64
COND, rel, glorot = R.COND, R.rel, R.glorot
IN, OUT = 5, 6


# ---- the hop and the two convolutions ------------------------------------------------------------------------------------------------
def hop(s, t, n_dst, z, w=None, ss=None, sd=None, alpha=1.0, beta=0.0, self_=None, gam=0.0, prev=None, add=None):
    """poly_conv_ref.hop, statement by statement, on torch tensors"""
    m = z[s]
    if ss is not None:
        m = m * ss[:, None]
    if w is not None:
        m = w[:, None] * m
    r = torch.zeros((n_dst, z.shape[1]), dtype=z.dtype).index_add(0, t, m)
    if sd is not None:
        r = r * sd[:, None]
    r = alpha * r
    if self_ is not None:
        r = r + beta * self_
    if prev is not None:
        r = r + gam * prev
    if add is not None:
        r = r + add
    return r


class Graph:
    """(s, t, n, w | None, λmax | None) with the degree vectors of both convolutions in `dtype`"""

    def __init__(self, s, t, n, w=None, lam=None, dtype=torch.float64):
        self.s, self.t, self.n = torch.as_tensor(np.asarray(s), dtype=torch.int64), torch.as_tensor(np.asarray(t), dtype=torch.int64), n
        self.w = None if w is None else torch.as_tensor(np.asarray(w)).to(dtype)
        self.lam, self.dtype = lam, dtype
        ww = None if w is None else np.asarray(w, f64)
        dout, din = np.bincount(s, weights=ww, minlength=n), np.bincount(t, weights=ww, minlength=n)
        self.deg_out, self.deg_in = torch.as_tensor(dout).to(dtype), torch.as_tensor(din).to(dtype)
        with np.errstate(divide="ignore"):
            self.c = torch.as_tensor(1 / np.sqrt(dout)).to(dtype)                  # R.cheb_c


def cheb_conv(G, x, W, b):
    """R.cheb_forward: W [K][out][in]"""
    a, bb = 2.0 / G.lam, 2.0 / G.lam - 1.0
    Z = [x]
    if len(W) > 1:
        Z.append(hop(G.s, G.t, G.n, x, G.w, G.c[G.s], G.c, -a, bb, x))
    for _ in range(2, len(W)):
        Z.append(hop(G.s, G.t, G.n, Z[-1], G.w, G.c[G.s], G.c, -2 * a, 2 * bb, Z[-1], -1.0, Z[-2]))
    Y = sum(Zk @ Wk.T for Zk, Wk in zip(Z, W))
    return Y if b is None else Y + b


def d_conv(G, x, W, b):
    """R.dconv_forward: W [2][k][out][in]; T0 is never advanced, slice 1 is read twice"""
    k = W.shape[1]
    idx = R.dconv_slices(k)
    S = (lambda T_, **kw: hop(G.t, G.s, G.n, T_, G.w, G.deg_in[G.t], **kw), lambda T_, **kw: hop(G.s, G.t, G.n, T_, G.w, G.deg_out[G.s], **kw))
    T = [[x], [x]]
    for d in (0, 1):
        if k > 1:
            T[d].append(S[d](x))
        for _ in range(1, k):
            T[d].append(S[d](T[d][-1], alpha=2.0, gam=-1.0, prev=x))
    h = sum(T[0][j] @ W[0, i].T + T[1][j] @ W[1, i].T for j, i in enumerate(idx))
    return h if b is None else h + b


def sigmoid(v):
    """NNlib's: t = exp(-|x|); x >= 0 ? 1 / (1 + t) : t / (1 + t)"""
    t = torch.exp(-v.abs())
    return torch.where(v >= 0, 1 / (1 + t), t / (1 + t))


# ---- the cells, as the reference wrote them (p: the tensors of cell.parameters(), in its order) -------------------------------------
def _rep(h, n, out, dtype):
    if h is None:
        h = torch.zeros(out, dtype=dtype)
    return h[None, :].expand(n, out) if h.dim() == 1 else h


def gconv_gru_cell(G, p, x, h):
    (Wxr, bxr, Whr, bhr), (Wxz, bxz, Whz, bhz), (Wxh, bxh, Whh, bhh) = p[0:4], p[4:8], p[8:12]
    h = _rep(h, G.n, Wxr.shape[1], x.dtype)
    r = sigmoid(cheb_conv(G, x, Wxr, bxr) + cheb_conv(G, h, Whr, bhr))
    z = sigmoid(cheb_conv(G, x, Wxz, bxz) + cheb_conv(G, h, Whz, bhz))
    ht = torch.tanh(cheb_conv(G, x, Wxh, bxh) + cheb_conv(G, r * h, Whh, bhh))
    h = (1 - z) * ht + z * h
    return h, h


def gconv_lstm_cell(G, p, x, state):
    h, c = state if state is not None else (None, None)
    gi, gf, gc, go = p[0:6], p[6:12], p[12:18], p[18:24]
    out = gi[0].shape[1]
    h, c = _rep(h, G.n, out, x.dtype), _rep(c, G.n, out, x.dtype)

    def pre(gt, cc):
        Wx, bx, Wh, bh, w, b = gt
        v = cheb_conv(G, x, Wx, bx) + cheb_conv(G, h, Wh, bh) + w * cc
        return v if b is None else v + b
    i = sigmoid(pre(gi, c))
    f = sigmoid(pre(gf, c))
    c = f * c + i * torch.tanh(pre(gc, c))
    o = sigmoid(pre(go, c))
    h = o * torch.tanh(c)
    return h, (h, c)


def dcgru_cell(G, p, x, h):
    Wu, bu, Wr, br, Wc, bc = p
    h = _rep(h, G.n, Wu.shape[2], x.dtype)
    ht = torch.cat([x, h], 1)
    z = sigmoid(d_conv(G, ht, Wu, bu))
    r = sigmoid(d_conv(G, ht, Wr, br))
    c = torch.tanh(d_conv(G, torch.cat([x, h * r], 1), Wc, bc))
    h = z * h + (1 - z) * c
    return h, h


CELLS = {"gconv_gru": gconv_gru_cell, "gconv_lstm": gconv_lstm_cell, "dcgru": dcgru_cell}


def scan(kind, G, p, x, state):
    """GNNRecurrence: x [N][T][in] -> [N][T][out]"""
    ys = []
    for t in range(x.shape[1]):
        y, state = CELLS[kind](G, p, x[:, t], state)
        ys.append(y)
    return torch.stack(ys, 1)


# ---- the graphs ------------------------------------------------------------------------------------------------------------------------
def ring_graph(n=16, isolated=False):
    """a directed ring with two chords, unweighted: in- and out-degrees at most 2 (DConv multiplies by the raw degree at every order); with
    `isolated` one more node without any edge"""
    s = list(range(n)) + [0, n // 2]
    t = [(i + 1) % n for i in range(n)] + [5 % n, (n // 2 + 5) % n]
    return np.array(s, np.int64), np.array(t, np.int64), n + int(isolated)


def graph_of(name):
    """(s, t, n, w | None, graph_sizes) of a named case graph; graph_sizes: the member sizes of a batch, else None"""
    if name == "bi":
        return (*R.bidirected_graph(), None, None)
    if name == "bi_w":                                       # asymmetric weights: the transposed operator differs
        return (*R.bidirected_graph(), R.cheb_weights("asymmetric"), None)
    if name == "bi2":                                        # a batch of two graphs
        s1, t1, n1 = R.bidirected_graph()
        s2, t2, n2 = R.bidirected_graph(n=11, extra=7, seed=5)
        return np.concatenate([s1, s2 + n1]), np.concatenate([t1, t2 + n1]), n1 + n2, None, (n1, n2)
    if name == "di_w":                                       # weighted degrees below 1
        s, t, n = R.directed_graph()
        return s, t, n, np.random.default_rng(31).uniform(0.1, 0.3, len(s)).astype(f32), None
    if name == "ring":
        return (*ring_graph(), None, None)
    if name == "ring_iso":
        return (*ring_graph(isolated=True), None, None)
    if name == "di_w2":                                      # a batch of two weighted directed graphs
        s1, t1, n1 = R.directed_graph()
        s2, t2, n2 = R.directed_graph(n=10, E=22, seed=6)
        w = np.random.default_rng(32).uniform(0.1, 0.3, len(s1) + len(s2)).astype(f32)
        return np.concatenate([s1, s2 + n1]), np.concatenate([t1, t2 + n1]), n1 + n2, w, (n1, n2)
    raise KeyError(name)


def lam_of(name):
    """λmax as the reference takes it (R.cheb_lam): eigmax of Symmetric(L), dense, float64"""
    s, t, n, w, _ = graph_of(name)
    A = np.zeros((n, n))
    np.add.at(A, (s, t), 1.0 if w is None else w.astype(f64))
    c = 1 / np.sqrt(A.sum(1))
    Lm = np.eye(n) - c[:, None] * A * c[None, :]
    return float(np.linalg.eigvalsh(np.triu(Lm) + np.triu(Lm, 1).T)[-1])


# ---- the layer cases: (kind, graph, k, T, bias, state, out) ------------------------------------------------------------------------------
STATES = ("none", "vec", "mat")


def _grid(kind, graphs):
    out = []
    for q, (k, T) in enumerate((k, T) for k in (1, 2, 3) for T in (1, 4)):
        gs = graphs if k < 3 or kind != "dcgru" else graphs[:1]      # unweighted DConv at k = 3, T = 4 is 1e-5 from float64: not a case
        out.append((kind, gs[q % len(gs)], k, T, q % 2 == 0, STATES[q % 3], OUT))
        out.append((kind, gs[(q + 1) % len(gs)], k, T, q % 2 == 1, STATES[(q + 1) % 3], OUT))
    return out


LAYER_CASES = (_grid("gconv_gru", ("bi", "bi_w")) + _grid("gconv_lstm", ("bi", "bi_w")) + _grid("dcgru", ("di_w", "ring"))
               + [("gconv_gru", "bi", 3, 2, True, "mat", 130), ("gconv_gru", "bi2", 2, 4, True, "vec", OUT),
                  ("gconv_lstm", "bi", 2, 2, True, "mat", 130), ("gconv_lstm", "bi2", 3, 4, False, "mat", OUT),
                  ("dcgru", "di_w", 2, 2, True, "mat", 130), ("dcgru", "ring_iso", 2, 4, True, "mat", OUT),
                  ("dcgru", "di_w2", 3, 4, False, "vec", OUT), ("dcgru", "ring_iso", 1, 4, True, "none", OUT)])


def case_id(c):
    kind, gname, k, T, bias, state, out = c
    return f"{kind}-{gname}-k{k}-T{T}-{'b' if bias else 'nob'}-{state}-o{out}"


def layer_case(c, seed=0):
    """dict(x [N][T][in], params (cell.parameters() order; None for a missing bias), state (tuple of arrays | None each), dy) float32"""
    kind, gname, k, T, bias, state, out = c
    n = graph_of(gname)[2]
    rng = np.random.default_rng([seed, sum(map(ord, kind + gname)), k, T, int(bias), STATES.index(state), out, 41])
    vec = lambda m: (0.1 * rng.standard_normal(m)).astype(f32)      # noqa: E731
    params = []
    if kind == "dcgru":
        for _ in range(3):
            params += [np.stack([np.stack([glorot(rng, out, IN + out) for _ in range(k)]) for _ in range(2)]), vec(out) if bias else None]
    else:
        for _ in range(3 if kind == "gconv_gru" else 4):
            params += [np.stack([glorot(rng, out, IN) for _ in range(k)]), vec(out) if bias else None,
                       np.stack([glorot(rng, out, out) for _ in range(k)]), vec(out) if bias else None]
            if kind == "gconv_lstm":
                params += [glorot(rng, out, 1).reshape(out), vec(out) if bias else None]

    def st():
        return None if state == "none" else (0.5 * rng.standard_normal(out if state == "vec" else (n, out))).astype(f32)
    states = (st(), st()) if kind == "gconv_lstm" else (st(),)
    return dict(x=rng.standard_normal((n, T, IN)).astype(f32), params=params, state=states,
                dy=rng.standard_normal((n, T, out)).astype(f32))


_REF = {}


def layer_ref(c, lam=None, dtype=f64):
    """dict(y, dx, dstate (list), dparams (list, None where the parameter is)) of the loss Σ y ⊙ dy in `dtype`; computed once per
    (case, λmax, dtype) and shared.  lam: λmax for the Chebyshev cells (None: lam_of)"""
    kind, gname = c[0], c[1]
    if kind != "dcgru" and lam is None:
        lam = lam_of(gname)
    key = (c, lam, dtype)
    if key in _REF:
        return _REF[key]
    td = torch.float64 if dtype == f64 else torch.float32
    s, t, n, w, _ = graph_of(gname)
    G = Graph(s, t, n, w, lam, td)
    case = layer_case(c)
    leaf = lambda a: None if a is None else torch.from_numpy(a).to(td).requires_grad_()      # noqa: E731
    x, p, st = leaf(case["x"]), [leaf(a) for a in case["params"]], [leaf(a) for a in case["state"]]
    state = (st[0], st[1]) if kind == "gconv_lstm" else st[0]
    if kind == "gconv_lstm" and st[0] is None:
        state = None
    y = scan(kind, G, p, x, state)
    wrt = [x] + [a for a in st if a is not None] + [a for a in p if a is not None]
    gr = list(torch.autograd.grad(y, wrt, torch.from_numpy(case["dy"]).to(td)))
    dx = gr.pop(0)
    dst = [None if a is None else gr.pop(0) for a in st]
    dp = [None if a is None else gr.pop(0) for a in p]
    npy = lambda a: None if a is None else a.detach().numpy()      # noqa: E731
    _REF[key] = dict(y=npy(y), dx=npy(dx), dstate=[npy(a) for a in dst], dparams=[npy(a) for a in dp])
    return _REF[key]


def flat(ref):
    """[(name, array)] of everything a layer_ref holds"""
    out = [("y", ref["y"]), ("dx", ref["dx"])]
    out += [(f"dstate{k}", a) for k, a in enumerate(ref["dstate"]) if a is not None]
    out += [(f"dparam{k}", a) for k, a in enumerate(ref["dparams"]) if a is not None]
    return out


def layer_condition(c):
    got, ref = flat(layer_ref(c, dtype=f32)), flat(layer_ref(c, dtype=f64))
    return max(rel(a, b) for (_, a), (_, b) in zip(got, ref))


# ---- the gate kernels: include/gnnmp.h's formulas in float64 numpy -----------------------------------------------------------------------
GATE_DS, GATE_NS, GATE_T, GATE_TS = (1, 5, 64, 130), (1, 37), 3, (0, 2)
H_KINDS = ("mat", "vec", "null")


def np_sigmoid(v):
    t = np.exp(-np.abs(v))
    return np.where(v >= 0, 1 / (1 + t), t / (1 + t))


def gate_case(cell, N, D, seed=0):
    """float32 operands of one gate-kernel call at T = GATE_T: everything either cell reads, each drawn independently"""
    G = 3 if cell == "gru" else 4
    rng = np.random.default_rng([seed, G, N, D, 43])
    nrm = lambda *sh: rng.standard_normal(sh).astype(f32)      # noqa: E731
    T = GATE_T
    ops = dict(P=nrm(N, T, G * D), a=nrm(N, G * D), h=nrm(N, D), hvec=nrm(D), dy=nrm(N, T, D), carry=nrm(N, D), carry2=nrm(N, 2 * D),
               drh=nrm(N, 2 * D), carry_c=nrm(N, D), w=(0.5 * nrm(4, D)), cnew_in=nrm(N, T, D))
    return ops


def state_of(ops, kind, N, D, dtype=f64):
    if kind == "null":
        return np.zeros((N, D), dtype)
    return (ops["h"] if kind == "mat" else np.broadcast_to(ops["hvec"], (N, D))).astype(dtype)


def gru_forward(ops, hkind, t, dtype=f64):
    """dict(r, z, rh, c, hn) [N][D] of both phases; phase 1's a is ops['a'][:, 2D:3D]"""
    P, a = ops["P"].astype(dtype), ops["a"].astype(dtype)
    N, D = a.shape[0], a.shape[1] // 3
    h = state_of(ops, hkind, N, D, dtype)
    Pt = P[:, t]
    r = np_sigmoid(Pt[:, :D] + a[:, :D])
    z = np_sigmoid(Pt[:, D:2 * D] + a[:, D:2 * D])
    c = np.tanh(Pt[:, 2 * D:] + a[:, 2 * D:])
    return dict(r=r, z=z, rh=r * h, c=c, hn=(1 - z) * c + z * h)


def gru_backward(ops, hkind, t, rep, carries, dtype=f64):
    """dict(dc, dz, dr, part1, part) of the pullback from the forward's gates; carries: which of (carry, carry2) are given"""
    f = gru_forward(ops, hkind, t, dtype)
    N, D = f["r"].shape
    h = state_of(ops, hkind, N, D, dtype)
    g = ops["dy"].astype(dtype)[:, t]
    if carries[0]:
        g = g + ops["carry"].astype(dtype)
    if carries[1]:
        for j in range(rep):
            g = g + ops["carry2"].astype(dtype)[:, j * D:(j + 1) * D]
    r, z, c = f["r"], f["z"], f["c"]
    dc = (g * (1 - z)) * (1 - c * c)
    dz = (g * (h - c)) * (z * (1 - z))
    part1 = g * z
    q = sum(ops["drh"].astype(dtype)[:, j * D:(j + 1) * D] for j in range(rep))
    dr = (q * h) * (r * (1 - r))
    return dict(dc=dc, dz=dz, dr=dr, part1=part1, part=part1 + q * r, **f)


def gate_condition(cell, N, D, t, kind):
    """the worst norm-wise distance of the float32 restatement from float64 over the outputs the GPU tests compare (an output that is
    exactly zero in both — h = 0 — counts as 0)"""
    ops = gate_case(cell, N, D)
    worst = 0.0
    runs = [(rep, car) for rep in (1, 2) for car in ((True, True), (False, False), (False, True))] if cell == "gru" else \
        [(1, car) for car in ((True, True), (False, False), (True, False))]
    for rep, car in runs:
        a, b = [gru_backward(ops, kind, t, rep, car, dt) if cell == "gru" else lstm_backward(ops, kind, t, car, dt) for dt in (f32, f64)]
        for k in b:
            if np.any(b[k] != 0):
                worst = max(worst, rel(a[k], b[k]))
    return worst


def lstm_forward(ops, ckind, t, dtype=f64):
    P, a, w = ops["P"].astype(dtype), ops["a"].astype(dtype), ops["w"].astype(dtype)
    N, D = a.shape[0], a.shape[1] // 4
    c = state_of(ops, ckind, N, D, dtype)
    pre = lambda q, cc: P[:, t, q * D:(q + 1) * D] + a[:, q * D:(q + 1) * D] + w[q] * cc      # noqa: E731
    i, f, g = np_sigmoid(pre(0, c)), np_sigmoid(pre(1, c)), np.tanh(pre(2, c))
    cn = f * c + i * g
    o = np_sigmoid(pre(3, cn))
    return dict(i=i, f=f, g=g, o=o, cn=cn, hn=o * np.tanh(cn), c=c)


def lstm_backward(ops, ckind, t, carries, dtype=f64):
    """carries: which of (carry_h, carry_c) are given; carry_h is ops['carry']"""
    F = lstm_forward(ops, ckind, t, dtype)
    w = ops["w"].astype(dtype)
    i, f, g, o, cn, c = F["i"], F["f"], F["g"], F["o"], F["cn"], F["c"]
    dh = ops["dy"].astype(dtype)[:, t]
    if carries[0]:
        dh = dh + ops["carry"].astype(dtype)
    th = np.tanh(cn)
    d_o = (dh * th) * (o * (1 - o))
    dcn = (dh * o) * (1 - th * th)
    if carries[1]:
        dcn = dcn + ops["carry_c"].astype(dtype)
    dcn = dcn + d_o * w[3]
    d_i, d_f, d_g = (dcn * g) * (i * (1 - i)), (dcn * c) * (f * (1 - f)), (dcn * i) * (1 - g * g)
    dc = dcn * f + d_i * w[0] + d_f * w[1] + d_g * w[2]
    return dict(da=np.concatenate([d_i, d_f, d_g, d_o], 1), dc=dc, peep=np.concatenate([d_i * c, d_f * c, d_g * c, d_o * cn], 1), **F)
