"""The cases of the GATConv edge-feature training exports (csrc/gat_backward.hip, csrc/gat_fused.hip) for the ABI's memory contract, kept
beside tests/abi_cases.py instead of in it: that module is a yardstick and stays as it is.  Importing this module registers
  gnnmp_gat_conv_edge_stats_f32, gnnmp_gat_conv_edge_grad_f32, gnnmp_gat_edge_fold_f32, gnnmp_gat_edge_fold_grad_f32   in TABLE
(they only launch), wrapped for the variants as the registry wraps its own builders.  As with tests/topk_cases.py, the registry knows
them in a session that has imported this module (tests/test_gat_edge_abi.py does, so a run of the whole suite has them when the
completeness guard executes); the parametrised tests of tests/test_abi_memory_contract.py and tests/test_abi_graph_capture.py take their
export lists before that, so tests/test_gat_edge_abi.py runs the same checks over these cases itself.

The graphs (one square relation of 37 nodes, one bipartite relation of 5 sources and 37 destinations, each also without any edge):
about 150 edges in short rows, (s, t) pairs listed several times — each listing carries its own edge score —, an explicit self edge, rows
without in-edges and sources without out-edges, a row of 9 edges, a row of 70 (more than one 64-slot stretch of a whole wave) and a row
of twice the plan's long-row threshold plus 5, which the plan chunks; a source whose out-edges exceed the threshold, so that the
transposed plan chunks a row too.  (H, C) are abi_cases.HC; the pair that does not fit a wave, (2, 33), is a refusal.

The reference is tests/gat_edge_grad_ref.py in float64; outputs owe the table's 1e-5 of its scale (abi_cases.compare).  Where the
reference is a difference of terms that cancel — dz = α (g - D) on a row whose edges carry equal values — the floor of "its scale" is the
size of the cancelling terms, per row, exactly as the registry states it for the e-less pullback (abi_cases.attn_ref: gscale)."""
import numpy as np

import abi_cases as A
import gat_edge_grad_ref as R

STATS, GRAD, FOLD, FOLD_GRAD = ("gnnmp_gat_conv_edge_stats_f32", "gnnmp_gat_conv_edge_grad_f32", "gnnmp_gat_edge_fold_f32",
                                "gnnmp_gat_edge_fold_grad_f32")
LAUNCH_ONLY = (STATS, GRAD, FOLD, FOLD_GRAD)
N, N_SRC_BI = 37, 5
ROW9, ROW70, ROW_LONG, SELF, HUB_SRC = 3, 11, 20, 25, 30            # destinations (and, for SELF and HUB_SRC, sources) with a role
EMPTY_DST = (0, 18, N - 1)                                           # rows without in-edges: first, interior, last
SLOPE = 0.2
f32, f64 = np.float32, np.float64


def long_len(thr):
    return 2 * int(thr) + 5


def _relation(name, n_src, thr, seed):
    """1-based (s, t) of the relation described above, edges in random order; the same for every variant (its own generator)"""
    rng = np.random.default_rng(seed)
    square = n_src == N
    special = {ROW9: 9, ROW70: 70, ROW_LONG: long_len(thr)}
    short = [i for i in range(N) if i not in special and i not in EMPTY_DST]
    t = np.concatenate([rng.choice(short, 150)] + [np.full(k, i) for i, k in special.items()])
    # sources: the last one of a bipartite relation / three nodes of the square one have no out-edge
    silent = {0, n_src - 1} if not square else {1, 18, N - 2}         # (source 0 of the bipartite relation gets its few edges below)
    talk = np.array([j for j in range(n_src) if j not in silent])
    s = rng.choice(talk, len(t))
    if square:
        pick = rng.permutation(len(t))[: thr + 9]                    # one source of more than thr out-edges: a chunked row of plan_t
        s[pick] = HUB_SRC
        k = int(np.flatnonzero(t == SELF)[0]) if (t == SELF).any() else 0
        t[k], s[k] = SELF, SELF                                      # an explicit self edge
    else:
        s[rng.permutation(len(t))[:7]] = 0                           # a short row of plan_t; sources 1, 2, 3 have more than thr out-edges
    rows = np.flatnonzero(t == ROW9)
    s[rows[:4]] = s[rows[0]]                                         # one (s, t) pair listed four times, another twice
    s[rows[5]] = s[rows[4]]
    perm = rng.permutation(len(t))
    s, t = s[perm], t[perm]
    g = A.Graph(name, s + 1, t + 1, n_src, N, thr=int(thr), want_split=int((np.bincount(t, minlength=N) > thr).sum()))
    return g


def graphs(ctx):
    """(square, bipartite, square without edges, bipartite without edges), made once per Ctx (plans are keyed on the Graph object)"""
    if "gat_edge" not in ctx.cache:
        ctx.cache["gat_edge"] = (_relation("ge_sq", N, ctx.thr, 71), _relation("ge_bi", N_SRC_BI, ctx.thr, 72),
                                 A.Graph("ge_sq0", [], [], N), A.Graph("ge_bi0", [], [], N_SRC_BI, N))
    return ctx.cache["gat_edge"]


def fits_wave(H, C):
    vec = 4 if C % 4 == 0 else 2 if C % 2 == 0 else 1
    return H * C // vec <= 64


def shapes(ctx):
    """(graph, bipartite?, H, C, tags, status)"""
    sq, bi, sq0, bi0 = graphs(ctx)
    for k, (H, C, tags) in enumerate(A.HC):
        if not fits_wave(H, C):
            yield sq, False, H, C, set(), A.EUNSUPPORTED             # a row wider than a wave: refused, nothing written
            continue
        yield sq, False, H, C, set(tags) | ({"ws"} if k == 0 else set()), A.OK
        yield bi, True, H, C, ({"align"} if k == 2 else set()) | ({"ws"} if k == 1 else set()), A.OK
    yield sq0, False, 3, 7, set(), A.OK
    yield bi0, True, 5, 4, set(), A.OK


def _operands(export, g, bip, H, C):
    r = A.rng_of(export, g.name, H, C)
    D = H * C
    return dict(Wx_src=A.F(r, g.n_src, D), Wx_dst=A.F(r, g.n_dst, D) if bip else None, a=A.F(r, H, 2 * C), es=A.F(r, g.E, H),
                bias=A.F(r, D), dout=A.F(r, g.n_dst, D))


def _core(g, i, H, C):
    sh = lambda v: None if v is None else v.astype(f64).reshape(-1, H, C)      # noqa: E731
    args = (g.s - 1, g.t - 1, g.n_src, g.n_dst, sh(i["Wx_src"]), sh(i["Wx_dst"]), i["a"].astype(f64), i["es"].astype(f64), SLOPE)
    o, c = R.core(*args)
    return o, c, args


def build_stats(ctx):
    for k, (g, bip, H, C, tags, status) in enumerate(shapes(ctx)):
        i = _operands(STATS, g, bip, H, C)
        D = H * C
        with_b, act, want_stats = k % 2 == 0, (k // 2) % 2, k % 3 != 1
        ref = None
        if status == A.OK:
            o, c, _ = _core(g, i, H, C)
            out = A.act64(act, o.reshape(g.n_dst, D) + (i["bias"].astype(f64) if with_b else 0.0))
            stats = np.stack([c["m"], c["den"]], -1)
            ne = g.indeg() > 0

            def ref(host, v=(out, stats, ne), want_stats=want_stats):
                # an empty row's (m, den) is written, but the header gives it no value
                return {"out": v[0], **({"stats": A.E(v[1], rows=v[2])} if want_stats else {})}
        args = [A.Pl(g), A.Arr("Wx_src", "in", i["Wx_src"]), A.Arr("Wx_dst", "in", i["Wx_dst"]) if bip else None, A.Arr("a", "in", i["a"]),
                A.Arr("edge_score", "in", i["es"]) if g.E else None, SLOPE, A.Arr("bias", "in", i["bias"]) if with_b else None, act,
                A.Arr("out", "out", shape=(g.n_dst, D)), A.Arr("stats", "out", shape=(g.n_dst, H, 2)) if want_stats else None, H, C, A.STREAM]
        yield A.mk(STATS, f"{g.name}_H{H}_C{C}", tags, args, ref, status=status)


def floors(g, i, c, gr):
    """the size of the terms that cancel inside dz = α (g - D), times the O(1) factors every gradient entry multiplies it with: per
    destination row, per source row, per edge and over all (abi_cases.attn_ref states the same floors for the e-less pullback)"""
    s, t = g.s - 1, g.t - 1
    big = max([1.0] + [float(np.abs(v).max()) for v in (i["a"], i["Wx_src"], i["Wx_dst"]) if v is not None and v.size])
    term = big * (np.abs(c["al"] * gr["g"]) + np.abs(c["al"] * gr["D"][t])).max(-1) if g.E else np.zeros(0)
    row_t, row_s = np.zeros(g.n_dst), np.zeros(g.n_src)
    np.maximum.at(row_t, t, term)
    np.maximum.at(row_s, s, term)
    return term, row_t, row_s


def build_grad(ctx):
    for k, (g, bip, H, C, tags, status) in enumerate(shapes(ctx)):
        i = _operands(GRAD, g, bip, H, C)
        D = H * C
        want_da = k % 3 != 1
        ref, stats = None, np.zeros((g.n_dst, H, 2), f32)
        if status == A.OK:
            o, c, args = _core(g, i, H, C)
            gr = R.core_grad(*args, c, i["dout"].astype(f64).reshape(-1, H, C))
            stats = np.stack([c["m"], c["den"]], -1).astype(f32)
            term, row_t, row_s = floors(g, i, c, gr)
            want = {"dsd": A.E(gr["dsd"], scale=row_t), "dss": A.E(gr["dss"], scale=row_s),
                    "dWx_src": A.E(gr["dWx_src"].reshape(-1, D), scale=row_s if bip else row_s + row_t)}      # Wx_dst NULL: both halves land in one row
            if bip:
                want["dWx_dst"] = A.E(gr["dWx_dst"].reshape(-1, D), scale=row_t)
            if want_da:
                want["da"] = A.E(gr["da"], scale=float(term.max()) if g.E else 0.0)
            if g.E:
                want["dscore"] = A.E(gr["des"], scale=term)
            ref = lambda host, want=want: dict(want)      # noqa: E731
        job = A.Rec("gnnmp_gat_edge_grad_t", Wx_src=A.Arr("Wx_src", "in", i["Wx_src"]), Wx_dst=A.Arr("Wx_dst", "in", i["Wx_dst"]) if bip else None,
                    a=A.Arr("a", "in", i["a"]), edge_score=A.Arr("edge_score", "in", i["es"]) if g.E else None, stats=A.Arr("stats", "in", stats),
                    dout=A.Arr("dout", "in", i["dout"]), line=A.Arr("line", "scratch", shape=(g.n_dst, H, 4)), dsd=A.Arr("dsd", "out", shape=(g.n_dst, H)),
                    dss=A.Arr("dss", "out", shape=(g.n_src, H)), dWx_src=A.Arr("dWx_src", "out", shape=(g.n_src, D)),
                    dWx_dst=A.Arr("dWx_dst", "out", shape=(g.n_dst, D)) if bip else None, da=A.Arr("da", "out", shape=(H, 2 * C)) if want_da else None,
                    dscore=A.Arr("dscore", "out", shape=(g.E, H)) if g.E else None, negative_slope=SLOPE)
        yield A.mk(GRAD, f"{g.name}_H{H}_C{C}", tags, [A.Pl(g), A.Pl(g, T=True), job, H, C, A.STREAM], ref, status=status,
                   align_status=A.LINE_ALIGN)


FOLD_SHAPES = tuple((H, C, ein, tags) for (H, C, tags), ein in zip(A.HC, (3, 1, 12, 1, 5, 130)))


def build_fold(ctx):
    for H, C, ein, tags in FOLD_SHAPES:
        r = A.rng_of(FOLD, H, C, ein)
        a_e, W_e = A.F(r, H, C), A.F(r, H * C, ein)
        yield A.mk(FOLD, f"H{H}_C{C}_e{ein}", tags, [A.Arr("a_e", "in", a_e), A.Arr("W_e", "in", W_e), A.Arr("M", "out", shape=(H, ein)), H, C, ein, A.STREAM],
                   lambda host, v=(a_e, W_e): {"M": R.fold(*v)})


def build_fold_grad(ctx):
    for k, (H, C, ein, tags) in enumerate(FOLD_SHAPES):
        r = A.rng_of(FOLD_GRAD, H, C, ein)
        a_e, W_e, dM = A.F(r, H, C), A.F(r, H * C, ein), A.F(r, H, ein)
        want_w, want_a = k % 3 != 1, k % 3 != 2

        def ref(host, v=(a_e, W_e, dM), want_w=want_w, want_a=want_a):
            dW, da = R.fold_grad(*v)
            return {**({"dW_e": dW} if want_w else {}), **({"da_e": da} if want_a else {})}
        yield A.mk(FOLD_GRAD, f"H{H}_C{C}_e{ein}_w{int(want_w)}a{int(want_a)}", tags,
                   [A.Arr("a_e", "in", a_e), A.Arr("W_e", "in", W_e), A.Arr("dM", "in", dM), A.Arr("dW_e", "out", shape=(H * C, ein)) if want_w else None,
                    A.Arr("da_e", "out", shape=(H, C)) if want_a else None, H, C, ein, A.STREAM], ref)


BUILDERS = {STATS: build_stats, GRAD: build_grad, FOLD: build_fold, FOLD_GRAD: build_fold_grad}

for _name, _build in BUILDERS.items():
    if _name not in A.TABLE:
        A.TABLE[_name] = A._of_variant(_build)          # as the registry's last lines wrap every builder it holds
