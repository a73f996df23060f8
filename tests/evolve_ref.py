"""EvolveGCNO restated from the Julia text in torch, any dtype (float64 is the reference; the float32 run of the same code gives the
CONDITION of a case): GraphNeuralNetworks/src/layers/temporalconv.jl:678-705 (the cell), :10-19 (scan over snapshots), Flux.LSTMCell
(gate order input, forget, cell, output) and GNNlib's gcn_conv (conv.jl:14-72: self loops, c = 1 ./ sqrt.(in-degree) on both sides, W
first when out < in).  Differentiable by autograd, which is where the reference gradients come from.  Plus the three kernels of
csrc/evolve.hip in numpy float64, and the cases the GPU tests run."""
import numpy as np
import torch

COND = 2e-6
PAIRS = [(2, 3), (3, 5), (8, 8), (13, 20), (20, 13), (33, 32), (32, 33)]
VARIANTS = ["init", "state", "nobias"]      # state = None; a state given; bias = false (state = None)
LAYER_CASES = [(cin, out, 3 + k % 3, v) for k, (cin, out) in enumerate(PAIRS) for v in VARIANTS]
STEP_DS = [1, 6, 15, 64, 260, 1056]


def case_id(c):
    return f"{c[0]}to{c[1]}_T{c[2]}_{c[3]}"


def sigmoid(x):
    return torch.sigmoid(x)


def lstm_cell(x, h, c, Wi, Wh, b):
    """Flux.LSTMCell: (h', c') from the input x and the state (h, c), all vectors"""
    a = Wi @ x + Wh @ h
    if b is not None:
        a = a + b
    i, f, g, o = a.chunk(4)
    cn = sigmoid(f) * c + sigmoid(i) * torch.tanh(g)
    return sigmoid(o) * torch.tanh(cn), cn


def gcn_conv(s, t, n, x, W, b):
    """gcn_conv with add_self_loops = true, no edge weights, identity σ; s, t 0-based LongTensors, x [n, in], W [out, in]"""
    loops = torch.arange(n)
    s2, t2 = torch.cat([s, loops]), torch.cat([t, loops])
    deg = torch.zeros(n, dtype=x.dtype).index_add(0, t2, torch.ones(len(t2), dtype=x.dtype))
    c = deg ** -0.5
    out, cin = W.shape
    if out < cin:
        x = x @ W.T
    m = x[s2] * c[s2][:, None]
    x = torch.zeros((n, x.shape[1]), dtype=x.dtype).index_add(0, t2, m) * c[:, None]
    if out >= cin:
        x = x @ W.T
    return x if b is None else x + b


def initial_weight(conv_w):
    """reshape(conv.weight, :) in Julia's column-major order: index o + out * i"""
    return conv_w.T.reshape(-1)


def weight_matrix(weight, cin, out):
    """reshape(weight, (out, in)), column-major"""
    return weight.reshape(cin, out).T


def cell_step(snap, x, conv_w, conv_b, Wi, Wh, b, state):
    """temporalconv.jl:701-705: (y, (weight, (h, c)))"""
    out, cin = conv_w.shape
    weight, (h, c) = state
    h, c = lstm_cell(weight, h, c, Wi, Wh, b)
    s, t, n = snap
    return gcn_conv(s, t, n, x, weight_matrix(h, cin, out), conv_b), (h, (h, c))


def model(snaps, xs, conv_w, conv_b, Wi, Wh, b, state=None):
    """scan (temporalconv.jl:10-19) of the cell over the snapshots: the list of y_t and the weights W_t [out, in] used"""
    out, cin = conv_w.shape
    if state is None:
        z = torch.zeros(cin * out, dtype=conv_w.dtype)
        state = (initial_weight(conv_w), (z, z))
    ys, Ws = [], []
    for snap, x in zip(snaps, xs):
        y, state = cell_step(snap, x, conv_w, conv_b, Wi, Wh, b, state)
        ys.append(y)
        Ws.append(weight_matrix(state[0], cin, out))
    return ys, Ws


def snapshots(cin, T, seed, same_nodes=None):
    """T snapshots with DIFFERENT node (5 .. 11) and edge counts, 1-based (s, t, n); snapshot 1 leaves its last node isolated"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(T):
        n = same_nodes if same_nodes is not None else 5 + (3 * k + seed) % 7
        E = n + 2 * k + 3
        hi = n - 1 if k == 1 else n
        s, t = rng.integers(0, hi, E), rng.integers(0, hi, E)
        out.append((s.astype(np.int64) + 1, t.astype(np.int64) + 1, n))
    return out


def layer_case(c, static=False):
    """the inputs of a case, numpy float32: weights uniform within the Glorot bound, biases within ±0.5, cotangents normal"""
    cin, out, T, variant = c
    seed = 1000 * cin + 10 * out + T
    rng = np.random.default_rng(seed)
    D = cin * out
    u = lambda bound, *shape: rng.uniform(-bound, bound, shape).astype(np.float32)      # noqa: E731
    bias = variant != "nobias"
    snaps = snapshots(cin, T, seed % 7, same_nodes=7 if static else None)
    case = dict(snaps=snaps, conv_w=u(np.sqrt(6 / (cin + out)), out, cin), conv_b=u(0.5, out) if bias else None,
                Wi=u(np.sqrt(6 / (5 * D)), 4 * D, D), Wh=u(np.sqrt(6 / (5 * D)), 4 * D, D), b=u(0.5, 4 * D) if bias else None,
                xs=[rng.standard_normal((n, cin)).astype(np.float32) for _, _, n in snaps],
                dys=[rng.standard_normal((n, out)).astype(np.float32) for _, _, n in snaps], state=None)
    if variant == "state":
        case["state"] = (u(np.sqrt(6 / (cin + out)), D), u(0.5, D), u(0.5, D))
    return case


PARAM_NAMES = ("conv_w", "conv_b", "Wi", "Wh", "b")


def run_case(case, dtype):
    """(ys, Ws, grads): the model and the gradient of Σ_t <y_t, dy_t> w.r.t. every x_t, the parameters and a given state, as float64
    numpy arrays, computed in `dtype`"""
    T_ = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=dtype).requires_grad_()      # noqa: E731
    snaps = [(torch.from_numpy(s - 1), torch.from_numpy(t - 1), n) for s, t, n in case["snaps"]]
    xs = [T_(x) for x in case["xs"]]
    par = {k: T_(case[k]) for k in PARAM_NAMES}
    st = None if case["state"] is None else [T_(a) for a in case["state"]]
    ys, Ws = model(snaps, xs, par["conv_w"], par["conv_b"], par["Wi"], par["Wh"], par["b"], None if st is None else (st[0], (st[1], st[2])))
    loss = sum((y * torch.tensor(dy, dtype=dtype)).sum() for y, dy in zip(ys, case["dys"]))
    wrt = {f"x{t}": x for t, x in enumerate(xs)}
    wrt.update({k: v for k, v in par.items() if v is not None and not (k == "conv_w" and st is not None)})
    if st is not None:
        wrt.update(dict(zip(("weight", "h", "c"), st)))
    grads = dict(zip(wrt, torch.autograd.grad(loss, list(wrt.values()))))
    n64 = lambda a: a.detach().to(torch.float64).numpy()      # noqa: E731
    return [n64(y) for y in ys], [n64(W) for W in Ws], {k: n64(v) for k, v in grads.items()}


def layer_condition(c):
    """the worst norm-wise distance of the float32 run from the float64 run over y and every gradient of a case"""
    case = layer_case(c)
    y32, _, g32 = run_case(case, torch.float32)
    y64, _, g64 = run_case(case, torch.float64)
    rel = lambda a, b: np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)      # noqa: E731
    return max([rel(a, b) for a, b in zip(y32, y64)] + [rel(g32[k], g64[k]) for k in g64])


# ---- the kernels of csrc/evolve.hip, numpy float64 -------------------------------------------------------------------------------------
def _sg(x):
    return 1.0 / (1.0 + np.exp(-x))


def step_inputs(D, seed=0):
    """Wi, Wh [4D][D] within ±1 / sqrt(D) (pre-activations of order one), x, h, c within ±1, b within ±0.5"""
    rng = np.random.default_rng(100 + D + seed)
    s = 1.0 / np.sqrt(D)
    return dict(Wi=rng.uniform(-s, s, (4 * D, D)).astype(np.float32), Wh=rng.uniform(-s, s, (4 * D, D)).astype(np.float32),
                x=rng.uniform(-1, 1, D).astype(np.float32), h=rng.uniform(-1, 1, D).astype(np.float32),
                c=rng.uniform(-1, 1, D).astype(np.float32), b=rng.uniform(-0.5, 0.5, 4 * D).astype(np.float32),
                da=rng.standard_normal(4 * D).astype(np.float32), add_x=rng.standard_normal(D).astype(np.float32),
                add_h=rng.standard_normal(D).astype(np.float32))


def step_ref(p, has_h=True, has_c=True, has_b=True, dtype=np.float64):
    """(h', c', a) of gnnmp_lstm_matvec_cell_f32"""
    f = lambda k: p[k].astype(dtype)      # noqa: E731
    a = f("Wi") @ f("x")
    if has_h:
        a = a + f("Wh") @ f("h")
    if has_b:
        a = a + f("b")
    D = len(p["x"])
    c = f("c") if has_c else np.zeros(D, dtype)
    cn = _sg(a[D:2 * D]) * c + _sg(a[:D]) * np.tanh(a[2 * D:3 * D])
    return _sg(a[3 * D:]) * np.tanh(cn), cn, a


def grad_ref(p):
    """(Wi' da, Wh' da) of gnnmp_lstm_matvec_grad_f32, without the addends"""
    da = p["da"].astype(np.float64)
    return p["Wi"].astype(np.float64).T @ da, p["Wh"].astype(np.float64).T @ da


def outer_ref(A, B):
    A, B = A.astype(np.float64), B.astype(np.float64)
    return A.T @ B, A.sum(0)
