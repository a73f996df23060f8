"""The cases of gnnmp_hetero_attn_f32 (csrc/hetero_attn.hip) for the ABI's memory contract, kept beside tests/abi_cases.py instead of in it:
that module is a yardstick and stays as it is.  Importing this module registers the export in A.TABLE (it only launches), wrapped for the
variants as the registry wraps its own builders; as with tests/gat_edge_cases.py, the registry knows it in a session that has imported
this module (tests/test_hetero_attn_abi.py does), and tests/test_hetero_attn_abi.py runs the registry's checks over these cases itself.

The relations (0-based roles; the edges of every relation are listed in random order, the same for every variant):
  into type B, 41 rows (no multiple of any rows-per-block count 4 .. 256):
    main   23 sources.  Rows 0, 20 and 40 are empty in EVERY relation; row 12 is empty here only.  Row lengths 1, 3, 4, 5 (U - 1, U, U + 1
           for U = 4), 2, 3, 5, 9, 17, 33, 65 (G + 1 for every group width G = 1 .. 64) and one row of 300 edges (simply long: the plans here
           are built with the library's own threshold); the rest 0 .. 6 at random.
    one    a single source (n_src = 1): every edge reads row 0 of K; row 13 is empty here only.
    none   five sources, no edge at all.
    rand   17 sources, 90 random edges (rows 0, 20, 40 kept empty).
  into type A, 7 rows: from the 41 nodes of B, 30 random edges.
  into type Z, 0 rows: from five sources, no edge.
The reference is tests/hetero_attn_ref.py in float64; every output owes the table's 1e-5 of its scale (abi_cases.compare)."""
import numpy as np

import abi_cases as A
import hetero_attn_ref as R

EXPORT = "gnnmp_hetero_attn_f32"
NB, NA = 41, 7
EMPTY_ALL = (0, 20, 40)
LENGTHS = {1: 1, 2: 3, 3: 4, 4: 5, 5: 2, 6: 9, 7: 17, 8: 33, 9: 65, 10: 300, 11: 3, 12: 0}
HC = ((1, 1), (2, 3), (1, 7), (4, 8), (8, 16), (4, 64))      # one lane; v = 1, an odd head; a single odd head; v = 4; 32 lanes; 64 lanes
SLOPE = 0.2
SUM, MAX, MIN = 0, 2, 3
COMBINE_NAME = {SUM: "+", MAX: "max", MIN: "min"}
f32 = np.float32


def _shuffled(name, s, t, n_src, n_dst, seed):
    perm = np.random.default_rng(seed).permutation(len(t))
    return A.Graph(name, np.asarray(s, np.int64)[perm] + 1, np.asarray(t, np.int64)[perm] + 1, n_src, n_dst)


def _graphs():
    rng = np.random.default_rng(41)
    deg = rng.integers(0, 7, NB)
    for i, k in LENGTHS.items():
        deg[i] = k
    deg[list(EMPTY_ALL)] = 0
    t = np.repeat(np.arange(NB), deg)
    main = _shuffled("hattn_main", rng.integers(0, 23, len(t)), t, 23, NB, 1)
    deg1 = rng.integers(0, 4, NB)
    deg1[list(EMPTY_ALL) + [13]] = 0
    t1 = np.repeat(np.arange(NB), deg1)
    one = _shuffled("hattn_one", np.zeros(len(t1), np.int64), t1, 1, NB, 2)
    none = A.Graph("hattn_none", [], [], 5, NB)
    live = np.array([i for i in range(NB) if i not in EMPTY_ALL])
    rand = _shuffled("hattn_rand", rng.integers(0, 17, 90), rng.choice(live, 90), 17, NB, 3)
    to_a = _shuffled("hattn_to_a", rng.integers(0, NB, 30), rng.integers(0, NA, 30), NB, NA, 4)
    to_z = A.Graph("hattn_to_z", [], [], 5, 0)
    return dict(main=main, one=one, none=none, rand=rand, to_a=to_a, to_z=to_z)


_G = {}


def graphs(ctx=None):
    """the relations, made once per Ctx (plans are keyed on the Graph object) — or once for the module when no Ctx is given"""
    cache = _G if ctx is None else ctx.cache
    if "hattn" not in cache:
        cache["hattn"] = _graphs()
    return cache["hattn"]


def rel(g, mode=R.GAT, bias=False, stats=False, act=0, a_scale=1.0):
    """one relation of a destination's table; g None: an identity relation"""
    return dict(g=g, mode=mode, bias=bias, stats=stats, act=act, a_scale=a_scale)


def draw(dsts, H, C, *key):
    """float inputs for a call: dsts = [(name, n_dst, combine, [rel(...)])] -> the same with Q, K, a, bias arrays in every relation"""
    r = A.rng_of("hetero_attn", H, C, *key)
    D = H * C
    out = []
    for name, n_dst, combine, rels in dsts:
        rs = []
        for x in rels:
            x = dict(x)
            g = x["g"]
            x["K"] = A.F(r, n_dst if g is None else g.n_src, D)
            if g is not None:
                x["Q"] = A.F(r, n_dst, D)
                x["a"] = (A.F(r, H, 2 * C if x["mode"] == R.GAT else C) * f32(x["a_scale"])).astype(f32)
                x["bias_v"] = A.F(r, D) if x["bias"] else None
            rs.append(x)
        out.append((name, n_dst, combine, rs))
    return out


def reference(dsts, H, C):
    """{array name: float64 reference} for every output of the call"""
    want = {}
    for name, n_dst, combine, rels in dsts:
        spec = [dict(s=None, K=x["K"]) if x["g"] is None else
                dict(s=x["g"].s - 1, t=x["g"].t - 1, mode=x["mode"], Q=x["Q"], K=x["K"], a=x["a"], bias=x["bias_v"], slope=SLOPE, act=x["act"])
                for x in rels]
        out, stats = R.hetero_attn(spec, n_dst, COMBINE_NAME[combine], H, C)
        want[f"out_{name}"] = out
        for j, (x, st) in enumerate(zip(rels, stats)):
            if x["g"] is not None and x["stats"]:
                want[f"stats_{name}{j}"] = st
    return want


def case(sid, tags, dsts, H, C, status=A.OK, align_status=None):
    """the registry's Case of one call on drawn data (draw)"""
    D = H * C
    recs = []
    for name, n_dst, combine, rels in dsts:
        tab = []
        for j, x in enumerate(rels):
            k = f"{name}{j}"
            if x["g"] is None:
                tab.append(A.Rec("gnnmp_hetero_attn_rel_t", plan=None, mode=0, Q=None, K=A.Arr(f"K_{k}", "in", x["K"], field="K"), a=None, bias=None,
                                 stats=None, negative_slope=0.0, act=0))
                continue
            tab.append(A.Rec("gnnmp_hetero_attn_rel_t", plan=A.Pl(x["g"]), mode=x["mode"], Q=A.Arr(f"Q_{k}", "in", x["Q"], field="Q"),
                             K=A.Arr(f"K_{k}", "in", x["K"], field="K"), a=A.Arr(f"a_{k}", "in", x["a"], field="a"),
                             bias=A.Arr(f"bias_{k}", "in", x["bias_v"], field="bias") if x["bias"] else None,
                             stats=A.Arr(f"stats_{k}", "out", shape=(n_dst, H, 2), field="stats") if x["stats"] else None,
                             negative_slope=SLOPE, act=x["act"]))
        recs.append(A.Rec("gnnmp_hetero_attn_dst_t", out=A.Arr(f"out_{name}", "out", shape=(n_dst, D), field="out"), n_dst=n_dst, combine=combine,
                          n_rel=len(tab), rels=tab))
    want = reference(dsts, H, C) if status == A.OK else {}
    return A.mk(EXPORT, sid, tags, [recs, len(recs), H, C, A.STREAM], lambda host, want=want: {k: A.E(v, "rel") for k, v in want.items()},
                status=status, align_status=align_status, no_warmup=True)


def table_dsts(G, k):
    """the k-th table of the cycle: GAT and GATv2 mixed at B, an identity relation first on even k, the fold, act, bias and stats cycling"""
    comb = (SUM, MAX, MIN)[k % 3]
    rels = [rel(None)] if k % 2 == 0 else []
    rels += [rel(G["main"], R.GAT if k % 2 else R.GATV2, bias=k % 2 == 0, stats=True, act=k % 2),
             rel(G["one"], R.GATV2 if k % 2 else R.GAT, bias=k % 2 == 1, stats=k % 2 == 1, act=(k + 1) % 2),
             rel(G["none"], R.GAT, bias=True, stats=True, act=0),
             rel(G["rand"], R.GATV2, bias=False, stats=k % 2 == 0, act=1)]
    return [("B", NB, comb, rels), ("A", NA, (SUM, MAX, MIN)[(k + 1) % 3], [rel(G["to_a"], R.GAT if k % 2 == 0 else R.GATV2, bias=True, stats=True, act=k % 2)]),
            ("Z", 0, SUM, [rel(G["to_z"], R.GAT, stats=True)])]


def sixteen_dsts(G):
    """16 records in one call: B takes twelve relations, A three, Z one"""
    names = ("main", "one", "none", "rand")
    rels = [rel(G[names[j % 4]], (R.GAT, R.GATV2)[(j // 2) % 2], bias=j % 3 == 0, stats=j % 5 == 0, act=j % 2) for j in range(12)]
    return [("B", NB, SUM, rels), ("A", NA, MAX, [rel(G["to_a"], R.GATV2), rel(None), rel(G["to_a"], R.GAT, bias=True, act=1)]),
            ("Z", 0, SUM, [rel(G["to_z"], R.GATV2)])]


def _build(ctx):
    G = graphs(ctx)
    for k, (H, C) in enumerate(HC):
        tags = set()
        if k == 0:
            tags.add("side")
        if (H, C) in ((2, 3), (4, 8)):      # rows of 6 and 32 floats: every shift still fits a wave at v = 1
            tags.add("align")
        if (H, C) == (4, 8):
            tags.add("ws")
        yield case(f"tab{k}_H{H}_C{C}", tags, draw(table_dsts(G, k), H, C, "table", k), H, C)
    yield case("sixteen_H4_C8", (), draw(sixteen_dsts(G), 4, 8, "sixteen"), 4, 8)


if EXPORT not in A.TABLE:
    A.TABLE[EXPORT] = A._of_variant(_build)          # as the registry's last lines wrap every builder it holds
