"""The recurrent layers of GraphNeuralNetworks/src/layers/temporalconv.jl: TGCN, and — further down, with headers of their own —
GConvGRU, GConvLSTM and DCGRU, then EvolveGCNO.

  TGCNCell       temporalconv.jl:809-849   conv_g = GNNChain(GCNConv(in => out, relu; kws...), GCNConv(out => out; kws...)) and
                                           dense_g = Dense(2out => out, σ | tanh) for g in z, r, h; one step
                                             z = dense_z(vcat(conv_z(g, x), h)),  r = dense_r(vcat(conv_r(g, x), h)),
                                             h~ = dense_h(vcat(conv_h(g, x), r .* h)),  h = (1 .- z) .* h .+ z .* h~;  returns (h, h)
  GNNRecurrence  temporalconv.jl:121-135   scans the cell over the time dimension: torch [N, T, in] -> [N, T, out]
  TGCN           temporalconv.jl:884       GNNRecurrence(TGCNCell(args...))

The graph convolutions never see the state, so the spatial work of all T steps and all three gates runs up front in a number of launches
independent of T (phase A: the time steps are columns — [N, T, C] is node-major, so one propagate at width T C serves every step — and the
three chains are stacked side by side, width 3 out).  What is left is node-local, and gnnmp_tgcn_recurrence_f32 runs all T steps in one
launch (csrc/temporal.hip).  For out > 128, or with knob 20 (KNOB_TGCN) < 0, the recurrence runs step by step instead: two gnnmp_dense_f32
products and two pointwise launches per step.

Weights keep the Julia shapes (GCNConv weight (out, in), Dense weight (out, 2out)); every arithmetic step is a libgnnmp call.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L
from .graph import GNNGraph, check_num_nodes
from .layers import Dense, GCNConv, GNNChain, dense, gcn_norm_cache
from .temporal_graph import TemporalSnapshotsGNNGraph

TGCN_MAX_OUT = 128          # the one-launch recurrence's envelope (csrc/temporal.hip)


class TGCNCell:
    """TGCNCell(in => out; bias=true, add_self_loops=true, use_edge_weight=false) — temporalconv.jl:809-849.  Fields as in the
    reference: in_ (`in` is a Python keyword), out, conv_z / conv_r / conv_h (GNNChain of two GCNConv), dense_z / dense_r / dense_h
    (Dense(2out => out)).  cell(g, x [N, in], h=None) -> (h, h) with h [N, out]; a state h may be [N, out] or [out] (repeated over the
    nodes); None is initialstates, zeros(out)."""

    takes_graph = True

    def __init__(self, ch, bias=True, add_self_loops=True, use_edge_weight=False, device="cuda", seed=None):
        cin, cout = ch
        s = 0 if seed is None else int(seed)
        self.in_, self.out = cin, cout
        kw = dict(bias=bias, add_self_loops=add_self_loops, use_edge_weight=use_edge_weight, device=device)
        for k, (name, sigma) in enumerate((("z", torch.sigmoid), ("r", torch.sigmoid), ("h", torch.tanh))):
            conv = GNNChain(GCNConv((cin, cout), "relu", seed=s + 10 * k + 1, **kw), GCNConv((cout, cout), seed=s + 10 * k + 2, **kw))
            setattr(self, "conv_" + name, conv)
            setattr(self, "dense_" + name, Dense((2 * cout, cout), sigma, device=device, seed=s + 10 * k + 3))

    @property
    def add_self_loops(self):
        return bool(self.conv_z.layers[0].add_self_loops)

    @property
    def use_edge_weight(self):
        return bool(self.conv_z.layers[0].use_edge_weight)

    def parameters(self):
        """the 18 parameter tensors in tgcn_ad's order: per gate z, r, h — conv layer 1 (weight, bias), conv layer 2 (weight, bias),
        dense (weight, bias); a bias is None with bias=false"""
        out = []
        for name in ("z", "r", "h"):
            c1, c2 = getattr(self, "conv_" + name).layers
            d = getattr(self, "dense_" + name)
            out += [c1.weight, c1.bias, c2.weight, c2.bias, d.weight, d.bias]
        return out

    def initialstates(self, device=None):
        return torch.zeros(self.out, dtype=torch.float32, device=device or self.dense_z.weight.device)

    def __call__(self, g, x, h=None):
        y = tgcn_forward(self, g, x.reshape(x.shape[0], 1, x.shape[-1]), h)
        h = y.reshape(y.shape[0], self.out)
        return h, h


class GNNRecurrence:
    """GNNRecurrence(cell) — temporalconv.jl:121-135: layer(g, x [N, T, in], state=None) -> [N, T, out], the cell scanned over the
    time dimension (the reference's dims = 2 of (in, T, N)); with a TemporalSnapshotsGNNGraph and a list of x_t [N_t, in] it returns the
    list of y_t [N_t, out] (the reference's second scan method, :10-19): a step-by-step loop for every cell but EvolveGCNOCell, which
    takes its fast path in both forms."""

    takes_graph = True

    def __init__(self, cell):
        self.cell = cell

    def __call__(self, g, x, state=None):
        if isinstance(self.cell, EvolveGCNOCell):
            return evolve_forward(self.cell, g, x, state)[0]
        if isinstance(g, TemporalSnapshotsGNNGraph):
            # the reference's second scan method (temporalconv.jl:10-19): snapshot t with x[t] [N_t, in]; a list of y_t [N_t, out]
            name = f"GNNRecurrence({type(self.cell).__name__})"
            if not isinstance(x, (list, tuple)):
                raise TypeError(f"{name}: with a TemporalSnapshotsGNNGraph x is a list of one feature array a snapshot")
            if len(x) != g.num_snapshots:
                raise ValueError(f"{name}: {len(x)} feature arrays for {g.num_snapshots} snapshots")
            ys = []
            for gt, xt in zip(g.snapshots, x):
                yt, state = self.cell(gt, xt, state)
                ys.append(yt)
            return ys
        if isinstance(self.cell, TGCNCell):
            return tgcn_forward(self.cell, g, x, state)
        if isinstance(self.cell, (GConvGRUCell, GConvLSTMCell, DCGRUCell)):
            return recurrent_forward(self.cell, g, x, state)[0]
        ys = []
        for t in range(x.shape[1]):
            yt, state = self.cell(g, x[:, t], state)          # the reference's order: (output, state)
            ys.append(yt)
        return torch.stack(ys, 1)


def TGCN(ch, **kw):
    """TGCN(in => out; kws...) = GNNRecurrence(TGCNCell(in => out; kws...)) — temporalconv.jl:884"""
    return GNNRecurrence(TGCNCell(ch, **kw))


# ---------------------------------------------------------------------------------------------------------
# shared pieces of the forward and the pullback (gnnmp/backward_temporal.py)
# ---------------------------------------------------------------------------------------------------------
def _blockdiag(ms):
    """[3out, 3out] with the three [out, out] blocks on the diagonal: the three gates' products as ONE dense launch over N T rows (the
    zeros add exact zeros; the products keep the reference's order — W_g[:, 1:out] is never pre-multiplied into W2_g)"""
    o = ms[0].shape[0]
    out = torch.zeros((3 * o, 3 * o), dtype=torch.float32, device=ms[0].device)
    for k, m in enumerate(ms):
        out[k * o:(k + 1) * o, k * o:(k + 1) * o] = m
    return out


def _cat_bias(bs):
    return None if bs[0] is None else torch.cat(bs).contiguous()


def stacked_params(cell):
    """(W1 [3out, in], b1, W2bd [3out, 3out], b2, Winbd [3out, 3out], bin, U_zr [2out, out], U_h [out, out]); bias None with bias=false"""
    o = cell.out
    c1 = [getattr(cell, "conv_" + n).layers[0] for n in "zrh"]
    c2 = [getattr(cell, "conv_" + n).layers[1] for n in "zrh"]
    d = [getattr(cell, "dense_" + n) for n in "zrh"]
    W1 = torch.cat([c.weight for c in c1]).contiguous()
    W2bd = _blockdiag([c.weight for c in c2])
    Winbd = _blockdiag([l.weight[:, :o] for l in d])
    Uzr = torch.cat([d[0].weight[:, o:], d[1].weight[:, o:]]).contiguous()
    Uh = d[2].weight[:, o:].contiguous()
    return W1, _cat_bias([c.bias for c in c1]), W2bd, _cat_bias([c.bias for c in c2]), Winbd, _cat_bias([l.bias for l in d]), Uzr, Uh


def gcn_propagate(g: GNNGraph, loops: bool, w, h, bias=None, relu=False):
    """GCNConv's normalised aggregation (GNNlib/src/layers/conv.jl:52-70, the norm caches gcn_conv uses) of [N, D] rows, D = T * C; with
    bias / relu the W-first branch's epilogue σ.(x .+ b) (b repeated over the T column blocks by the caller)"""
    plan = g.plan(loops)
    c, c_slot, w_slot = gcn_norm_cache(g, loops, w)
    out = torch.empty((plan.n_dst, h.shape[1]), dtype=torch.float32, device=h.device)
    lib = L.load()
    if bias is not None or relu:
        L.check(lib.gnnmp_propagate_slots_act_f32(plan.handle, L.SUM, L.ptr(h), L.ptr(w_slot), L.ptr(c_slot), L.ptr(c), L.ptr(bias),
                                                  L.ACT_RELU if relu else L.ACT_IDENTITY, L.ptr(out), h.shape[1], L.stream_ptr()))
    else:
        L.check(lib.gnnmp_propagate_slots_f32(plan.handle, L.SUM, L.ptr(h), L.ptr(w_slot), L.ptr(c_slot), L.ptr(c), L.ptr(out), h.shape[1],
                                              L.stream_ptr()))
    return out


def phase_a(cell, g: GNNGraph, x, sp):
    """the three GCN chains and the input halves of the three Dense layers for all T steps: P [N, T, 3out] and what the pullback needs
    (a dict).  Five to six launches whatever T is."""
    W1, b1, W2bd, b2, Winbd, bin_, _, _ = sp
    N, T, cin = x.shape
    o = cell.out
    loops = cell.add_self_loops
    w = g.w if cell.use_edge_weight else None
    xf = x.contiguous()
    sv = {}
    if o >= cin:
        # layer 1, aggregate first (conv.jl:59-71): one propagate of x as [N, T in], shared by the three gates (same normalisation)
        a1 = gcn_propagate(g, loops, w, xf.view(N, T * cin))
        h1 = dense(a1.view(N * T, cin), W1, b1, "relu")
        sv["a1"] = a1
    else:
        # W first (conv.jl:36-40): the stacked product, then one propagate at width T 3out with bias and relu in its epilogue
        u = dense(xf.view(N * T, cin), W1)
        h1 = gcn_propagate(g, loops, w, u.view(N, T * 3 * o), bias=None if b1 is None else b1.repeat(T), relu=True).view(N * T, 3 * o)
    a2 = gcn_propagate(g, loops, w, h1.view(N, T * 3 * o))
    C = dense(a2.view(N * T, 3 * o), W2bd, b2)
    P = dense(C, Winbd, bin_)
    sv.update(x=xf, h1=h1, a2=a2, C=C)
    return P.view(N, T, 3 * o), sv


def state_arg(h, N, out, device):
    """(tensor or None, stride) of a state: None -> zeros; [out] -> one vector for every node (stride 0); [N, out] -> per node"""
    if h is None:
        return None, out
    h = h.to(device=device, dtype=torch.float32).contiguous()
    if h.dim() == 1:
        if h.numel() != out:
            raise ValueError(f"state of size {h.numel()}, expected {out}")
        return h, 0
    if tuple(h.shape) != (N, out):
        raise ValueError(f"state of shape {tuple(h.shape)}, expected ({N}, {out}) or ({out},)")
    return h, out


def use_fused(out):
    return L.knob(L.KNOB_TGCN) >= 0 and out <= TGCN_MAX_OUT


def recurrence(P, Uzr, Uh, h0, h0_stride, need_gates=True):
    """y [N, T, out] (and the saved gates [N, T, 3out]) of the recurrence over P: one launch, or the per-step path"""
    N, T, D3 = P.shape
    o = D3 // 3
    lib = L.load()
    y = torch.empty((N, T, o), dtype=torch.float32, device=P.device)
    fused = use_fused(o)                                     # (one read of the knob per recurrence)
    gates = torch.empty((N, T, 3 * o), dtype=torch.float32, device=P.device) if (need_gates or not fused) else None
    if fused:
        L.check(lib.gnnmp_tgcn_recurrence_f32(L.ptr(P), L.ptr(Uzr), L.ptr(Uh), L.ptr(h0), h0_stride, L.ptr(y), L.ptr(gates), N, T, o,
                                              L.stream_ptr()))
        return y, gates
    h = torch.zeros((N, o), dtype=torch.float32, device=P.device) if h0 is None else h0.expand(N, o).contiguous()
    for t in range(T):
        a = dense(h, Uzr)
        rh = torch.empty((N, o), dtype=torch.float32, device=P.device)
        L.check(lib.gnnmp_tgcn_step_f32(0, L.ptr(P), L.ptr(a), L.ptr(h), o, L.ptr(gates), L.ptr(rh), None, N, T, t, o, L.stream_ptr()))
        a = dense(rh, Uh)
        hn = torch.empty((N, o), dtype=torch.float32, device=P.device)
        L.check(lib.gnnmp_tgcn_step_f32(1, L.ptr(P), L.ptr(a), L.ptr(h), o, L.ptr(gates), L.ptr(hn), L.ptr(y), N, T, t, o,
                                        L.stream_ptr()))
        h = hn
    return y, gates


# ---------------------------------------------------------------------------------------------------------
# GConvGRU, GConvLSTM, DCGRU — temporalconv.jl:143-293, 297-477, 480-613
#
# The x side of every gate and every step depends on x only: its Chebyshev / diffusion basis is built ONCE at width T in (the time steps
# are columns of [N][T in], as in TGCN's phase A) and one dense with the gate-stacked weights gives P [N][T][G out] with every bias
# folded in.  Per step the basis of the state is built by gnnmp_poly_hop_ld_f32 straight into the column blocks of a panel [N][B out],
# ONE dense over the panel with the gate-stacked weights follows, then one gate kernel (csrc/recurrent.hip), which writes h' (or r .* h)
# into block 0 of the panel that is read next.  Launches per step: GConvGRU 2K + 2, GConvLSTM K + 1, DCGRU 4k + 4 (k = 1: 4).
# Stacking weights is a copy made once per call, never arithmetic (the biases of one gate are added up: two or three [out] vectors).
# ---------------------------------------------------------------------------------------------------------
def _blk(panel, j, D):
    return panel[:, j * D:(j + 1) * D]


def poly_hop_ld(plan, z, alpha, w_slot=None, ss_slot=None, scale_dst=None, beta=0.0, self_=None, gamma=0.0, prev=None, add=None, out=None):
    """gnnmp_poly_hop_ld_f32 on column blocks: every operand a [rows][D] view whose last stride is 1 (its row stride is the panel's);
    out may be prev or add (the same view), never z or self_"""
    D = z.shape[1]
    if plan.n_dst == 0 or D == 0:
        return out
    ops = (z, self_, prev, add, out)
    assert all(o is None or (o.dim() == 2 and o.shape[1] == D and (o.stride(1) == 1 or D == 1) and o.dtype == torch.float32) for o in ops)
    ld = [D if o is None else (o.stride(0) if o.shape[0] > 1 else max(o.stride(0), D)) for o in ops]
    job = L.PolyHopLdJob(L.ptr(z), L.ptr(w_slot), L.ptr(ss_slot), L.ptr(scale_dst), L.ptr(self_), L.ptr(prev), L.ptr(add), float(alpha),
                         float(beta), float(gamma), L.ptr(out), ld[0], ld[1], ld[2], ld[3], ld[4])
    L.check(L.load().gnnmp_poly_hop_ld_f32(plan.handle, ctypes.byref(job), D, L.stream_ptr()))
    return out


class ChebBasis:
    """the Chebyshev basis of cheb_conv (conv.jl:83-98) on panels: block k of [N][K D] holds Z_{k+1}; `rep` = 1 (the state is block 0)"""

    rep = 1

    def __init__(self, g, K):
        from .backward import plan_transposed
        from .backward_poly import _slot_factors
        from .layers_more import scaled_laplacian_op
        self.K = self.B = K
        self.c, self.ss, self.ws, lam = scaled_laplacian_op(g)
        self.a, self.b = 2.0 / lam, 2.0 / lam - 1.0
        self.plan = g.plan(False)
        self.g, self._t, self._pt, self._sf = g, None, plan_transposed, _slot_factors

    def build(self, panel, D):
        """blocks 1 .. K - 1 from block 0: K - 1 launches"""
        a, b = self.a, self.b
        for k in range(1, self.K):
            z = _blk(panel, k - 1, D)
            if k == 1:
                poly_hop_ld(self.plan, z, -a, self.ws, self.ss, self.c, b, z, out=_blk(panel, 1, D))
            else:
                poly_hop_ld(self.plan, z, -2.0 * a, self.ws, self.ss, self.c, 2.0 * b, z, -1.0, _blk(panel, k - 2, D), out=_blk(panel, k, D))

    def pullback(self, G, D):
        """Clenshaw over the transposed plan, in place on the panel's cotangent (block k = G_{k+1}): afterwards block 0 is the cotangent
        of the state.  K - 1 launches."""
        if self.K == 1:
            return
        if self._t is None:
            pt = self._pt(self.g, False)
            self._t = (pt,) + tuple(self._sf(self.g, pt, "cheb_t", self.c))
        pt, sst, wst = self._t
        a, b = self.a, self.b
        for k in range(self.K - 1, 0, -1):                 # 1-based order k: G_k is block k - 1, B_{k+1} block k, B_{k+2} block k + 1
            z = _blk(G, k, D)
            prev = _blk(G, k + 1, D) if k + 1 < self.K else None
            two = 2.0 if k >= 2 else 1.0
            tgt = _blk(G, k - 1, D)
            poly_hop_ld(pt, z, -two * a, wst, sst, self.c, two * b, z, -1.0 if prev is not None else 0.0, prev, tgt, out=tgt)

    def block_slices(self):
        """the weight slice (a ChebConv's order) of each block"""
        return list(range(self.K))


class DiffusionBasis:
    """the diffusion basis of d_conv (conv.jl:696-724) on panels: DConv reads T_0 with one weight slice a direction, so the state is held
    in blocks 0 AND 1 (`rep` = 2); for k >= 2 the k terms T_1 .. T_k of direction 0 (the steps over gᵀ) follow in blocks 2 .., then those
    of direction 1.  T_0 is never advanced and weight slice 1 is read twice (d_conv_ad: _dconv_slices): the stacked weight repeats it."""

    rep = 2

    def __init__(self, g, k):
        from .backward_poly import _dconv_ops, _dconv_slices
        self.k = k
        self.B = 2 if k == 1 else 2 + 2 * k
        self.fwd, self.adj = _dconv_ops(g)
        self.idx = _dconv_slices(k)

    def _term(self, d, j):
        return 2 + d * self.k + (j - 1)

    def build(self, panel, D):
        """2k launches (k = 1: none)"""
        if self.k == 1:
            return
        t0 = _blk(panel, 0, D)
        for d in (0, 1):
            plan, ws, ss = self.fwd[d]
            poly_hop_ld(plan, t0, 1.0, ws, ss, out=_blk(panel, self._term(d, 1), D))
            for j in range(2, self.k + 1):
                poly_hop_ld(plan, _blk(panel, self._term(d, j - 1), D), 2.0, ws, ss, gamma=-1.0, prev=t0, out=_blk(panel, self._term(d, j), D))

    def pullback(self, G, D):
        """the adjoint recurrence of d_conv_ad in place: afterwards blocks 0 + 1 are the cotangent of the state.  2k launches, and for
        k >= 3 one gnnmp_add_f32 per further order and direction (Σ_{j >= 2} C_j, what the `- T_0` terms send back)."""
        if self.k == 1:
            return
        from .layers_more import _add
        t0 = _blk(G, 0, D)
        for d in (0, 1):
            plan, ws, sd = self.adj[d]
            C = _blk(G, self._term(d, self.k), D)
            R = None
            for j in range(self.k - 1, 0, -1):
                R = C if R is None else _add(R.contiguous(), C.contiguous())
                Gj = _blk(G, self._term(d, j), D)
                C = poly_hop_ld(plan, C, 2.0, ws, None, sd, add=Gj, out=Gj)
            poly_hop_ld(plan, C, 1.0, ws, None, sd, gamma=-1.0 if R is not None else 0.0, prev=R, add=t0, out=t0)

    def block_slices(self):
        """(direction, weight slice) of each block"""
        out = [(0, 0), (1, 0)]
        if self.k > 1:
            out += [(d, self.idx[j]) for d in (0, 1) for j in range(1, self.k + 1)]
        return out


def _check_cell_args(name, ch, k):
    cin, out = ch
    if int(cin) < 1 or int(out) < 1:
        raise ValueError(f"{name}: channels must be positive, got {cin} => {out}")
    if int(k) < 1:
        raise ValueError(f"{name}: k must be at least 1, got {k}")
    return int(cin), int(out), int(k)


class GConvGRUCell:
    """GConvGRUCell(in => out, k; bias = true) — temporalconv.jl:143-259.  Fields as in the reference: conv_x_r, conv_h_r, conv_x_z,
    conv_h_z, conv_x_h, conv_h_h (gnnmp.ChebConv), k, in_, out.  cell(g, x [N, in], h = None) -> (h', h'); a state is None
    (initialstates: zeros), [out] (repeated over the nodes) or [N, out]."""

    takes_graph = True
    gates = ("r", "z", "h")

    def __init__(self, ch, k, bias=True, device="cuda", seed=None):
        from .layers_more import ChebConv
        cin, out, k = _check_cell_args("GConvGRUCell", ch, k)
        s = 0 if seed is None else int(seed)
        self.in_, self.out, self.k = cin, out, k
        for j, n in enumerate(self.gates):
            setattr(self, "conv_x_" + n, ChebConv((cin, out), k, bias=bias, device=device, seed=s + 100 * j + 1))
            setattr(self, "conv_h_" + n, ChebConv((out, out), k, bias=bias, device=device, seed=s + 100 * j + 51))

    def parameters(self):
        """12 tensors in gconv_gru_ad's order: per gate r, z, h — conv_x (weight, bias), conv_h (weight, bias); a bias is None with
        bias = false"""
        out = []
        for n in self.gates:
            cx, chh = getattr(self, "conv_x_" + n), getattr(self, "conv_h_" + n)
            out += [cx.weight, cx.bias, chh.weight, chh.bias]
        return out

    def initialstates(self, device=None):
        return torch.zeros(self.out, dtype=torch.float32, device=device or self.conv_x_r.weight.device)

    def __call__(self, g, x, state=None):
        _, h, _, _ = recurrent_forward(self, g, x.reshape(x.shape[0], 1, x.shape[-1]), state)
        return h, h


class GConvLSTMCell:
    """GConvLSTMCell(in => out, k; bias = true) — temporalconv.jl:297-442.  Fields as in the reference: conv_x_g, conv_h_g
    (gnnmp.ChebConv), w_g [out] (the peephole, Julia (out, 1)) and b_g [out] (None with bias = false) for g in i, f, c, o; k, in_, out.
    cell(g, x [N, in], (h, c) = None) -> (h', (h', c')); h and c are each None, [out] or [N, out]."""

    takes_graph = True
    gates = ("i", "f", "c", "o")

    def __init__(self, ch, k, bias=True, device="cuda", seed=None):
        from .layers import glorot_uniform
        from .layers_more import ChebConv
        cin, out, k = _check_cell_args("GConvLSTMCell", ch, k)
        s = 0 if seed is None else int(seed)
        self.in_, self.out, self.k = cin, out, k
        for j, n in enumerate(self.gates):
            setattr(self, "conv_x_" + n, ChebConv((cin, out), k, bias=bias, device=device, seed=s + 100 * j + 1))
            setattr(self, "conv_h_" + n, ChebConv((out, out), k, bias=bias, device=device, seed=s + 100 * j + 51))
            setattr(self, "w_" + n, glorot_uniform(out, 1, device=device, seed=s + 100 * j + 91).reshape(out).contiguous())
            setattr(self, "b_" + n, torch.zeros(out, dtype=torch.float32, device=device) if bias else None)

    def parameters(self):
        """24 tensors in gconv_lstm_ad's order: per gate i, f, c, o — conv_x (weight, bias), conv_h (weight, bias), w, b"""
        out = []
        for n in self.gates:
            cx, chh = getattr(self, "conv_x_" + n), getattr(self, "conv_h_" + n)
            out += [cx.weight, cx.bias, chh.weight, chh.bias, getattr(self, "w_" + n), getattr(self, "b_" + n)]
        return out

    def initialstates(self, device=None):
        z = torch.zeros(self.out, dtype=torch.float32, device=device or self.conv_x_i.weight.device)
        return z, z.clone()

    def __call__(self, g, x, state=None):
        _, h, c, _ = recurrent_forward(self, g, x.reshape(x.shape[0], 1, x.shape[-1]), state)
        return h, (h, c)


class DCGRUCell:
    """DCGRUCell(in => out, k; bias = true) — temporalconv.jl:480-579.  Fields as in the reference: in_, out, k, dconv_u, dconv_r,
    dconv_c = gnnmp.DConv((in + out, out), k).  cell(g, x [N, in], h = None) -> (h', h')."""

    takes_graph = True
    gates = ("r", "u", "c")          # the kernels' order (r, z, c): u is the update gate z

    def __init__(self, ch, k, bias=True, device="cuda", seed=None):
        from .layers_more import DConv
        cin, out, k = _check_cell_args("DCGRUCell", ch, k)
        s = 0 if seed is None else int(seed)
        self.in_, self.out, self.k = cin, out, k
        for j, n in enumerate(("u", "r", "c")):
            setattr(self, "dconv_" + n, DConv((cin + out, out), k, bias=bias, device=device, seed=s + 1000 * j + 1))

    def parameters(self):
        """6 tensors in dcgru_ad's order: dconv_u (weights, bias), dconv_r (weights, bias), dconv_c (weights, bias)"""
        return [self.dconv_u.weights, self.dconv_u.bias, self.dconv_r.weights, self.dconv_r.bias, self.dconv_c.weights, self.dconv_c.bias]

    def initialstates(self, device=None):
        return torch.zeros(self.out, dtype=torch.float32, device=device or self.dconv_u.weights.device)

    def __call__(self, g, x, state=None):
        _, h, _, _ = recurrent_forward(self, g, x.reshape(x.shape[0], 1, x.shape[-1]), state)
        return h, h


def GConvGRU(ch, k, **kw):
    """GConvGRU(in => out, k; kws...) = GNNRecurrence(GConvGRUCell(...)) — temporalconv.jl:293"""
    return GNNRecurrence(GConvGRUCell(ch, k, **kw))


def GConvLSTM(ch, k, **kw):
    """GConvLSTM(in => out, k; kws...) = GNNRecurrence(GConvLSTMCell(...)) — temporalconv.jl:477"""
    return GNNRecurrence(GConvLSTMCell(ch, k, **kw))


def DCGRU(ch, k, **kw):
    """DCGRU(in => out, k; kws...) = GNNRecurrence(DCGRUCell(...)) — temporalconv.jl:613"""
    return GNNRecurrence(DCGRUCell(ch, k, **kw))


def _sum_bias(bs):
    """the biases of one gate added up (None with bias = false)"""
    from .layers_more import _add
    bs = [b for b in bs if b is not None]
    if not bs:
        return None
    tot = bs[0]
    for b in bs[1:]:
        tot = _add(tot, b)
    return tot


def cell_basis(cell, g):
    return DiffusionBasis(g, cell.k) if isinstance(cell, DCGRUCell) else ChebBasis(g, cell.k)


def cell_stacked(cell, basis):
    """(Wx [G out][B in], bias [G out] | None, Wh: list of state-side stacks [Gi out][B out]) — GRU cells: Wh = [r and z, candidate];
    the LSTM: Wh = [all four gates].  Block b of a stack is the weight slice basis.block_slices()[b]: copies, no arithmetic."""
    cin = cell.in_
    sl = basis.block_slices()
    wx, wh, bs = [], [], []
    for n in cell.gates:
        if isinstance(cell, DCGRUCell):
            W = getattr(cell, "dconv_" + n).weights                                  # [2][k][out][in + out]
            wx.append(torch.cat([W[d, i][:, :cin] for d, i in sl], 1))
            wh.append(torch.cat([W[d, i][:, cin:] for d, i in sl], 1))
            bs.append(getattr(cell, "dconv_" + n).bias)
        else:
            cx, chh = getattr(cell, "conv_x_" + n), getattr(cell, "conv_h_" + n)      # weight [K][out][*]
            wx.append(torch.cat([cx.weight[i] for i in sl], 1))
            wh.append(torch.cat([chh.weight[i] for i in sl], 1))
            bs.append(_sum_bias([cx.bias, chh.bias, getattr(cell, "b_" + n, None)]))
    Wx = torch.cat(wx).contiguous()
    bias = None if bs[0] is None else torch.cat(bs).contiguous()
    if isinstance(cell, GConvLSTMCell):
        return Wx, bias, [torch.cat(wh).contiguous()]
    return Wx, bias, [torch.cat(wh[:2]).contiguous(), wh[2].contiguous()]


def x_side(basis, x, Wx, bias):
    """P [N][T][G out] for all steps and the stacked basis Xb [N T][B in] it was made from: B - rep hops at width T in, one interleaving
    copy, one dense — whatever T is"""
    N, T, cin = x.shape
    W = T * cin
    Xp = torch.empty((N, basis.B * W), dtype=torch.float32, device=x.device)
    for j in range(basis.rep):
        _blk(Xp, j, W).copy_(x.reshape(N, W))
    basis.build(Xp, W)
    Xb = Xp.view(N, basis.B, T, cin).permute(0, 2, 1, 3).contiguous().view(N * T, basis.B * cin)
    P = dense(Xb, Wx, bias)
    return P.view(N, T, Wx.shape[0]), Xb


def _fill_state(panel, h0, stride, rep, D):
    for j in range(rep):
        if h0 is None:
            _blk(panel, j, D).zero_()
        else:
            _blk(panel, j, D).copy_(h0 if stride else h0.expand(panel.shape[0], D))


def _at(t, offset_floats):
    return ctypes.c_void_p(t.data_ptr() + 4 * offset_floats)


def _check_recurrent_input(name, cell, g, x):
    if isinstance(x, (tuple, list)):
        raise NotImplementedError(f"{name}: a bipartite (xs, xt) input is not covered; pass one feature array")
    if x.dtype != torch.float32:
        raise ValueError(f"{name}: the HIP kernels are Float32; x is {x.dtype}")
    if x.dim() != 3 or x.shape[2] != cell.in_:
        raise ValueError(f"{name}: x must be [N][T][{cell.in_}] for this layer, not {tuple(x.shape)}")
    check_num_nodes(g, x)


def recurrent_forward(cell, g: GNNGraph, x, state=None, keep=False):
    """(y [N, T, out], h_T [N, out], c_T | None) of GNNRecurrence(cell) for the three graph-convolutional cells; with `keep` also a dict of
    what the pullback needs (gnnmp/backward_recurrent.py): the panels of all steps, time-major, the gates, the x basis"""
    name = type(cell).__name__
    _check_recurrent_input(name, cell, g, x)
    N, T, _ = x.shape
    D = cell.out
    lstm = isinstance(cell, GConvLSTMCell)
    hs, cs0 = (state if state is not None else (None, None)) if lstm else (state, None)
    if lstm and state is not None and not (isinstance(state, (tuple, list)) and len(state) == 2):
        raise ValueError(f"{name}: the state is a pair (h, c)")
    h0, ldh0 = state_arg(hs, N, D, x.device)
    c0, ldc0 = state_arg(cs0, N, D, x.device) if lstm else (None, D)
    f32 = dict(dtype=torch.float32, device=x.device)
    basis = cell_basis(cell, g)
    Wx, bias, Wh = cell_stacked(cell, basis)
    P, Xb = x_side(basis, x.contiguous(), Wx, bias)
    B, rep = basis.B, basis.rep
    BD = B * D
    lib = L.load()
    G = 4 if lstm else 3
    y = torch.empty((N, T, D), **f32)
    gates = torch.empty((N, T, G * D), **f32)
    n1 = T if keep else min(T, 2)
    pan1 = torch.empty((n1, N, BD), **f32)                  # the basis of h_{t-1}: kept time-major for the weight gradients, else two
    _fill_state(pan1[0], h0, ldh0, rep, D)
    sv = dict(basis=basis, Wx=Wx, Wh=Wh, has_bias=bias is not None, Xb=Xb, gates=gates, pan1=pan1, h0=h0, ldh0=ldh0, c0=c0, ldc0=ldc0)
    if lstm:
        w = torch.stack([cell.w_i, cell.w_f, cell.w_c, cell.w_o]).contiguous()
        cs = torch.empty((N, T, D), **f32)
        sv.update(w=w, cs=cs)
        for t in range(T):
            p1 = pan1[t if keep else t % 2]
            basis.build(p1, D)
            a = dense(p1, Wh[0])
            cp, ldc = (_at(cs, (t - 1) * D), T * D) if t > 0 else (L.ptr(c0), ldc0)
            nxt = pan1[(t + 1) if keep else (t + 1) % 2] if t + 1 < T else None
            job = L.LstmCellJob(L.ptr(P), L.ptr(a), L.ptr(w), cp, ldc, L.ptr(gates), L.ptr(cs), L.ptr(nxt), BD, L.ptr(y))
            if N:
                L.check(lib.gnnmp_lstm_cell_f32(ctypes.byref(job), N, T, t, D, L.stream_ptr()))
        return y, y[:, T - 1], cs[:, T - 1], sv
    pan2 = torch.empty((T if keep else 1, N, BD), **f32)    # the basis of r .* h_{t-1}
    sv.update(pan2=pan2)
    for t in range(T):
        p1, p2 = pan1[t if keep else t % 2], pan2[t if keep else 0]
        basis.build(p1, D)
        a = dense(p1, Wh[0])
        job = L.GruCellJob(L.ptr(P), L.ptr(a), L.ptr(p1), BD, L.ptr(gates), L.ptr(p2), BD, rep, None)
        if N:
            L.check(lib.gnnmp_gru_cell_f32(0, ctypes.byref(job), N, T, t, D, L.stream_ptr()))
        basis.build(p2, D)
        a = dense(p2, Wh[1])
        nxt = pan1[(t + 1) if keep else (t + 1) % 2] if t + 1 < T else None
        job = L.GruCellJob(L.ptr(P), L.ptr(a), L.ptr(p1), BD, L.ptr(gates), L.ptr(nxt), BD, rep, L.ptr(y))
        if N:
            L.check(lib.gnnmp_gru_cell_f32(1, ctypes.byref(job), N, T, t, D, L.stream_ptr()))
    return y, y[:, T - 1], None, sv


def tgcn_forward(cell, g: GNNGraph, x, state=None):
    """GNNRecurrence(TGCNCell)(g, x [N, T, in], state) -> [N, T, out] (forward only; tgcn_ad differentiates it)"""
    if x.dim() != 3 or x.shape[2] != cell.in_:
        raise ValueError(f"TGCN input must be [N, T, {cell.in_}], got {tuple(x.shape)}")
    check_num_nodes(g, x)
    N, T, _ = x.shape
    sp = stacked_params(cell)
    P, _ = phase_a(cell, g, x.to(torch.float32), sp)
    h0, stride = state_arg(state, N, cell.out, x.device)
    y, _ = recurrence(P, sp[6], sp[7], h0, stride, need_gates=False)
    return y


# ---------------------------------------------------------------------------------------------------------
# EvolveGCNO — temporalconv.jl:678-752
#
# The cell's LSTM evolves the FLATTENED weight of its GCNConv (D = in out; Wi, Wh [4D][D]), at batch one: a step is two matrix-vector
# products over 8 D^2 floats and one launch of gnnmp_lstm_matvec_cell_f32 (csrc/evolve.hip).  The weight sequence depends on the
# parameters and the state only — never on x or the graph — so it is made first: Wseq [T + 1][D], row 0 the weight that entered, row t
# the weight of snapshot t.  The snapshots are independent given their weights: their normalised aggregation is ONE propagate over the
# block-diagonal batch (TemporalSnapshotsGNNGraph.batched), and the product with W_t one gnnmp_dense_f32 a snapshot on its contiguous row
# range, reading row t of Wseq in place: flattened in Julia's column-major order (index o + out i) a weight vector IS the [in][out]
# row-major matrix that gnnmp_dense_f32 reads with w_layout = 1.  2T + 1 launches for T snapshots.
# ---------------------------------------------------------------------------------------------------------
class LSTMCell:
    """Flux.LSTMCell(n_in => n_out; bias): Wi [4 n_out, n_in], Wh [4 n_out, n_out], b [4 n_out] or None; gate order input, forget, cell,
    output (as in Set2Set).  A bag of parameters: EvolveGCNOCell steps it with gnnmp_lstm_matvec_cell_f32."""

    def __init__(self, ch, bias=True, device="cuda", seed=None):
        from .layers import glorot_uniform
        n_in, n_out = ch
        s = 0 if seed is None else int(seed)
        self.in_, self.out = n_in, n_out
        self.Wi = glorot_uniform(4 * n_out, n_in, device=device, seed=s)
        self.Wh = glorot_uniform(4 * n_out, n_out, device=device, seed=s + 1)
        self.b = torch.zeros(4 * n_out, dtype=torch.float32, device=device) if bias else None


class EvolveGCNOCell:
    """EvolveGCNOCell(in => out; bias = true) — temporalconv.jl:678-705.  Fields as in the reference: in_, out, conv = GCNConv(in => out;
    bias) (identity σ, self loops, no edge weights), lstm = LSTMCell(in out => in out; bias).
    cell(g, x [N, in], state = None) -> (y [N, out], (weight, (h, c))): the LSTM advances the flattened weight, the convolution uses it.
    A state is (weight [D], (h [D], c [D])), D = in out; None is initialstates()."""

    takes_graph = True

    def __init__(self, ch, bias=True, device="cuda", seed=None):
        cin, out = ch
        if int(cin) < 1 or int(out) < 1:
            raise ValueError(f"EvolveGCNOCell: channels must be positive, got {cin} => {out}")
        s = 0 if seed is None else int(seed)
        self.in_, self.out = int(cin), int(out)
        self.conv = GCNConv((self.in_, self.out), bias=bias, device=device, seed=s + 1)
        D = self.in_ * self.out
        self.lstm = LSTMCell((D, D), bias=bias, device=device, seed=s + 2)

    def parameters(self):
        """5 tensors in evolve_gcno_ad's order: conv.weight [out, in], conv.bias, lstm.Wi, lstm.Wh, lstm.b; a bias is None with bias=false.
        in out + out + 8 D^2 + 4D numbers: 321 for 2 => 3, 696 for 3 => 3 (the reference docstring's figures)."""
        return [self.conv.weight, self.conv.bias, self.lstm.Wi, self.lstm.Wh, self.lstm.b]

    def initialstates(self):
        """(weight, (h, c)) — temporalconv.jl:693-697: weight = reshape(conv.weight, :), COLUMN-MAJOR as in Julia (index o + out i, i.e.
        conv.weight.T.reshape(-1)), which makes Wi, Wh and b interchangeable with the reference's; h and c zeros of length D"""
        w = self.conv.weight.t().reshape(-1)
        z = torch.zeros(self.in_ * self.out, dtype=torch.float32, device=w.device)
        return w, (z, z.clone())

    def __call__(self, g, x, state=None):
        x3 = x.reshape(x.shape[0], 1, x.shape[-1]) if torch.is_tensor(x) and x.dim() == 2 else x
        return evolve_forward(self, g, x3, state, name="EvolveGCNOCell", single=True)


def EvolveGCNO(ch, **kw):
    """EvolveGCNO(in => out; kws...) = GNNRecurrence(EvolveGCNOCell(...)) — temporalconv.jl:752.  layer(tg, [x_t [N_t, in]]) -> [y_t
    [N_t, out]] over a TemporalSnapshotsGNNGraph; layer(g, x [N, T, in]) -> [N, T, out] over a static graph, which runs as T copies of
    g through the same path (one block-diagonal propagate, cached on g per T)."""
    return GNNRecurrence(EvolveGCNOCell(ch, **kw))


def _check_evolve_x(name, cell, n_nodes, xt, what):
    if isinstance(xt, (tuple, list)):
        raise NotImplementedError(f"{name}: a bipartite (xs, xt) input is not covered; pass one feature array")
    if not torch.is_tensor(xt):
        raise TypeError(f"{name}: {what} is a {type(xt).__name__}, not a tensor")
    if xt.dtype != torch.float32:
        raise ValueError(f"{name}: the HIP kernels are Float32; {what} is {xt.dtype}")
    if xt.dim() != 2 or xt.shape[1] != cell.in_:
        raise ValueError(f"{name}: {what} must be [N][{cell.in_}] for this layer, not {tuple(xt.shape)}")
    if xt.shape[0] != n_nodes:
        raise ValueError(f"{name}: {what} has {xt.shape[0]} rows, its snapshot has {n_nodes} nodes")


def evolve_inputs(name, cell, g, x):
    """(tg, xcat [Σ N_t, in], static): both input forms brought to one — a temporal graph and the snapshots' features one under the
    other.  Static form: the T time slices of x [N, T, in] over T copies of g (the temporal graph is kept on g, one per T)."""
    if isinstance(g, TemporalSnapshotsGNNGraph):
        if not isinstance(x, (list, tuple)):
            raise TypeError(f"{name}: with a TemporalSnapshotsGNNGraph x is a list of one feature array a snapshot")
        if len(x) != g.num_snapshots:
            raise ValueError(f"{name}: {len(x)} feature arrays for {g.num_snapshots} snapshots")
        if g.num_snapshots == 0:
            raise ValueError(f"{name}: a temporal graph without snapshots")
        for t, xt in enumerate(x):
            _check_evolve_x(name, cell, g.num_nodes[t], xt, f"x[{t}]")
        return g, (x[0] if len(x) == 1 else torch.cat(list(x))).contiguous(), False
    if not isinstance(g, GNNGraph):
        raise TypeError(f"{name}: expected a GNNGraph or a TemporalSnapshotsGNNGraph, got {type(g).__name__}")
    if isinstance(x, (tuple, list)):
        raise NotImplementedError(f"{name}: a bipartite (xs, xt) input is not covered; pass one feature array")
    if x.dtype != torch.float32:
        raise ValueError(f"{name}: the HIP kernels are Float32; x is {x.dtype}")
    if x.dim() != 3 or x.shape[2] != cell.in_ or x.shape[1] < 1:
        raise ValueError(f"{name}: x must be [N][T][{cell.in_}] for this layer, not {tuple(x.shape)}")
    if x.shape[0] != g.num_nodes:
        raise ValueError(f"{name}: x has {x.shape[0]} rows, the graph has {g.num_nodes} nodes")
    N, T, cin = x.shape
    key = ("evolve_static", T)
    tg = g._cache.get(key)
    if tg is None:
        tg = g._cache[key] = TemporalSnapshotsGNNGraph([g] * T)
    return tg, x.permute(1, 0, 2).reshape(T * N, cin).contiguous(), True


def evolve_state(name, cell, state, device):
    """(weight0, h0, c0) of a given state, float32 and contiguous; (None, None, None) for None (initialstates)"""
    if state is None:
        return None, None, None
    D = cell.in_ * cell.out
    try:
        w0, (h0, c0) = state
    except (TypeError, ValueError):
        raise ValueError(f"{name}: the state is (weight, (h, c))") from None
    out = []
    for what, v in (("weight", w0), ("h", h0), ("c", c0)):
        if not torch.is_tensor(v) or v.numel() != D:
            raise ValueError(f"{name}: the state's {what} must have in * out = {D} elements")
        if v.dtype != torch.float32:
            raise ValueError(f"{name}: the HIP kernels are Float32; the state's {what} is {v.dtype}")
        out.append(v.to(device).reshape(D).contiguous())
    return tuple(out)


def evolve_weights(cell, T, w0, h0, c0, keep=False):
    """the weight sequence: (Wseq [T + 1][D], Cseq [T + 1][D], A [T][4D] | None).  Row 0 holds what entered (w0: None = the flattened
    conv.weight; c0: None = zeros), step t reads row t - 1 — as the LSTM's input and, from step 2 on, as its hidden state too — and
    writes row t: T launches.  `keep`: the pre-activations, for the pullback."""
    D = cell.in_ * cell.out
    lstm = cell.lstm
    dev = lstm.Wi.device
    f32 = dict(dtype=torch.float32, device=dev)
    Wseq, Cseq = torch.empty((T + 1, D), **f32), torch.empty((T + 1, D), **f32)
    Wseq[0].copy_(cell.conv.weight.t().reshape(-1) if w0 is None else w0)
    if c0 is None:
        Cseq[0].zero_()
    else:
        Cseq[0].copy_(c0)
    A = torch.empty((T, 4 * D), **f32) if keep else None
    lib = L.load()
    for t in range(1, T + 1):
        h = L.ptr(h0) if t == 1 else _at(Wseq, (t - 1) * D)
        job = L.LstmMatvecJob(L.ptr(lstm.Wi), L.ptr(lstm.Wh), _at(Wseq, (t - 1) * D), h, _at(Cseq, (t - 1) * D), L.ptr(lstm.b),
                              _at(Wseq, t * D), _at(Cseq, t * D), None if A is None else _at(A, (t - 1) * 4 * D))
        L.check(lib.gnnmp_lstm_matvec_cell_f32(ctypes.byref(job), D, L.stream_ptr()))
    return Wseq, Cseq, A


def dense_rows(x, r0, r1, Wflat, cin, out, w_layout, bias, dst):
    """dst[r0:r1] = x[r0:r1] * M (w_layout = 1, M = Wflat as [in][out]: [., in] -> [., out]) or x[r0:r1] * M' (w_layout = 0, M read as the
    [Dout = in][K = out] matrix: [., out] -> [., in]) (+ bias): one gnnmp_dense_f32 on a contiguous row range, the weight read in place"""
    if r1 <= r0:
        return
    K, Dout = (cin, out) if w_layout else (out, cin)
    assert x.shape[1] == K and dst.shape[1] == Dout and x.is_contiguous() and dst.is_contiguous()
    L.check(L.load().gnnmp_dense_f32(_at(x, r0 * K), L.ptr(Wflat), K, out, None, None, 0, 0, int(w_layout), L.ptr(bias), L.ACT_IDENTITY,
                                     _at(dst, r0 * Dout), r1 - r0, Dout, L.stream_ptr()))


def evolve_conv(cell, tg, xcat, Wseq):
    """(y [Σ N_t, out], agg | None): gcn_conv of every snapshot with its own weight, row t + 1 of Wseq for snapshot t.  out >= in:
    aggregate first (one propagate at width in, then T products, the bias in their epilogue; agg is what the ΔW of the pullback reads);
    out < in: W first (T products, then one propagate at width out with the bias in its epilogue), as gcn_conv does."""
    gb, seg = tg.batched()
    cin, out = cell.in_, cell.out
    conv = cell.conv
    T = tg.num_snapshots
    f32 = dict(dtype=torch.float32, device=xcat.device)
    if out >= cin:
        agg = gcn_propagate(gb, True, None, xcat)
        y = torch.empty((xcat.shape[0], out), **f32)
        for t in range(T):
            dense_rows(agg, seg[t], seg[t + 1], Wseq[t + 1], cin, out, 1, conv.bias, y)
        return y, agg
    u = torch.empty((xcat.shape[0], out), **f32)
    for t in range(T):
        dense_rows(xcat, seg[t], seg[t + 1], Wseq[t + 1], cin, out, 1, None, u)
    return gcn_propagate(gb, True, None, u, bias=conv.bias), None


def evolve_output(tg, y, static):
    """the caller's form back: a list of y_t [N_t, out], or [N, T, out] for the static form"""
    if static:
        T, N = tg.num_snapshots, tg.num_nodes[0]
        return y.view(T, N, y.shape[1]).permute(1, 0, 2).contiguous()
    return list(y.split(tg.num_nodes))


def evolve_forward(cell, g, x, state=None, name="EvolveGCNO", single=False):
    """(y, (weight_T, (h_T, c_T))) of GNNRecurrence(EvolveGCNOCell) in both input forms (evolve_inputs); `single`: one step of the
    cell on a plain graph, x [N, 1, in] -> y [N, out]"""
    if single and isinstance(g, TemporalSnapshotsGNNGraph):
        raise TypeError(f"{name}: a cell steps on one GNNGraph; scan a TemporalSnapshotsGNNGraph with EvolveGCNO / GNNRecurrence")
    tg, xcat, static = evolve_inputs(name, cell, g, x)
    if not (cell.conv.add_self_loops and not cell.conv.use_edge_weight and cell.conv.sigma is None):
        raise ValueError(f"{name}: the cell's GCNConv must be the reference's (identity σ, self loops, no edge weights)")
    w0, h0, c0 = evolve_state(name, cell, state, xcat.device)
    T = tg.num_snapshots
    Wseq, Cseq, _ = evolve_weights(cell, T, w0, h0, c0)
    y, _ = evolve_conv(cell, tg, xcat, Wseq)
    out = evolve_output(tg, y, static)
    if single:
        out = out.reshape(out.shape[0], cell.out)
    return out, (Wseq[T], (Wseq[T], Cseq[T]))


