"""The cases of the grouped dense exports (csrc/dense_grouped.hip) for the ABI's memory contract, beside tests/abi_cases.py as
tests/topk_cases.py is: importing this module registers both exports in TABLE (they only launch).  tests/test_grouped_dense_abi.py runs the
contract and capture checks over them; the float64 restatements, group by group, also serve tests/test_grouped_dense.py."""
import numpy as np

import abi_cases as A

FWD, GRAD = "gnnmp_grouped_dense_f32", "gnnmp_grouped_dense_grad_w_f32"
SIZES = (0, 1, 15, 16, 17, 0, 40, 3, 3, 3, 3, 70)      # empty groups in front and inside, a 16-row tile cut four times, a group over several tiles
seg_of = lambda sizes: np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)      # noqa: E731


# ---- the launch geometries of tests/test_grouped_dense_geometry.py; what tests/test_grouped_route_cpu.py expects of the planner at 256 CUs ----
# Ten groups with a mean of 83 rows: four waves a block, a super-tile of 64 rows.  Boundaries at 70, 90, 95, 105, 120 cut all four tiles of
# super-tile [64, 128); group 2 = [90, 95) lies inside wave 1's tile, group 3 is empty between groups 2 and 4, which share that tile;
# group 7 starts on 192 = 3 * 64, group 8 on 400 = 25 * 16 (no multiple of 64); the last tile is partial.  check_cut restates this.
CUT = (70, 20, 5, 0, 10, 15, 72, 208, 131, 300)
CUT_POISON = 2                                          # an interior group whose rows share a 16-row tile with both neighbours
SLABS4 = (1000, 0, 3, 5, 700, 1, 9, 330)                # S = 4 at 256 CUs: the groups of 3, 5, 1 and 9 rows leave empty and short slabs
SLABS4_POISON = 3
UNEVEN_1000 = (256, 0, 1, 255, 3, 0, 229, 27, 1, 228)   # 256 rows a block of the any-shape kernel: boundaries on, beside and inside the blocks
N40 = (7, 0, 1, 19, 13)


def check_cut(sizes, waves):
    """what the cut_multiwave cases rest on, for the `waves` the route reports (a super-tile is waves * 16 rows)"""
    seg, SR = seg_of(sizes), waves * 16
    starts = [(int(seg[g]), int(seg[g + 1])) for g in range(len(sizes))]
    inner = [int(b) for b in seg[1:-1] if b % 16]                                                  # boundaries strictly inside a 16-row tile
    assert any(all(any(b // SR == st and (b % SR) // 16 == w for b in inner) for w in range(waves)) for st in range(int(seg[-1]) // SR + 1)), \
        "no super-tile has a boundary inside the tile of each of its waves"
    assert any(e > s and s // 16 == (e - 1) // 16 and (s % SR) // 16 > 0 for s, e in starts), "no group inside the tile of a wave > 0"
    assert any(e > s > 0 and s % SR == 0 for s, e in starts), "no group starts on a super-tile boundary"
    assert any(e > s and s % 16 == 0 and s % SR for s, e in starts), "no group starts on a 16-row boundary inside a super-tile"
    assert any(s == e and 0 < g < len(sizes) - 1 and s % 16 and sizes[g - 1] and sizes[g + 1] for g, (s, e) in enumerate(starts)), \
        "no empty group between two groups that share a tile"
    return True


def uneven_sizes(N, G, seed):
    """G group sizes that add up to N: about a tenth empty, a few single rows, a few long groups, the rest exponential"""
    rng = np.random.default_rng(seed)
    w = rng.exponential(size=G)
    w[rng.random(G) < 0.1] = 0.0
    w[rng.integers(0, G, 5)] *= 20.0
    sizes = np.floor(w / w.sum() * (N - G)).astype(np.int64)
    sizes[(w > 0) & (rng.random(G) < 0.03)] = 1
    sizes[int(np.argmax(sizes))] += N - int(sizes.sum())
    assert sizes.min() == 0 and (sizes == 1).any() and sizes.sum() == N
    return tuple(int(v) for v in sizes)


ROUTE_T16, ROUTE_FMA, ROUTE_GRADW16, ROUTE_GRADW_FMA = 1, 2, 3, 4      # gnnmp.grouped: ROUTE_*
# (id, sizes, K, Dout, w_layout, bias, relu, pad, x_shift, why, at256): `sizes` a tuple or a callable (made when the case runs); `pad` floats
# behind every row of x and out (twice behind every W), `x_shift` floats x starts off 16 bytes; `why` names the property the test asserts
# from the route record; `at256` = (kernel, ncb, waves, tiles_per_block, grid_x, grid_y) of the planner at 256 CUs.
GEOM_FWD = [
    ("cut_multiwave_k20", CUT, 20, 12, 0, "group", 1, 4, 0, "multiwave", (ROUTE_T16, 2, 4, 1, 13, 1)),
    ("cut_multiwave_k24_d100", CUT, 24, 100, 1, "shared", 0, 0, 0, "multiwave", (ROUTE_T16, 7, 4, 1, 13, 1)),
    ("ncb4_d40", SIZES, 20, 40, 0, None, 0, 0, 0, "ncb4", (ROUTE_T16, 4, 1, 1, 11, 1)),
    ("ncb4_d52", SIZES, 20, 52, 1, "group", 1, 4, 0, "ncb4", (ROUTE_T16, 4, 1, 1, 11, 1)),
    ("ncb6_d72", SIZES, 20, 72, 0, "shared", 1, 0, 0, "ncb6", (ROUTE_T16, 6, 1, 1, 11, 1)),
    ("lds_stepdown_k320_d128", SIZES, 320, 128, 0, "group", 0, 0, 0, "stepdown", (ROUTE_T16, 7, 1, 1, 11, 2)),
    ("lds_stepdown_k640_d36", SIZES, 640, 36, 1, "group", 1, 4, 0, "stepdown", (ROUTE_T16, 2, 1, 1, 11, 2)),
    ("lds_none_fits_k1284", SIZES, 1284, 4, 0, "shared", 0, 0, 0, "fma_aligned", (ROUTE_FMA, 0, 0, 256, 1, 1)),
    ("persistent_small_groups", SIZES * 240, 4, 8, 0, "group", 1, 0, 0, "persistent", (ROUTE_T16, 2, 1, 2, 1283, 1)),
    ("persistent_lds_bound", SIZES * 30, 192, 112, 1, None, 0, 0, 0, "persistent", (ROUTE_T16, 7, 1, 2, 161, 1)),
    ("persistent_multiwave", lambda: uneven_sizes(200000, 500, 7), 4, 8, 1, "shared", 0, 0, 0, "persistent_multiwave", (ROUTE_T16, 2, 16, 2, 391, 1)),
    ("fma_multiblock_d132_shifted", SIZES, 20, 132, 0, "group", 1, 4, 1, "fma_multiblock", (ROUTE_FMA, 0, 0, 31, 6, 1)),
    ("fma_multiblock_2to3", UNEVEN_1000, 2, 3, 1, "shared", 0, 1, 1, "fma_multiblock", (ROUTE_FMA, 0, 0, 256, 4, 1)),
    ("fma_multiblock_d5000", N40, 3, 5000, 0, None, 1, 0, 0, "fma_multiblock", (ROUTE_FMA, 0, 0, 1, 40, 1)),
]
# (id, sizes, K, Dout, dW?, db, pad, shift, slabs, at256): `pad` floats behind the rows of dz and x and behind every dW[g], `shift` floats
# dz and x start off 16 bytes; `slabs` = the least S the case needs; at256 = (kernel, S, waves, tiles_per_wave, grid_x, grid_y, grid_z, fold_y)
GEOM_GRAD = [
    ("slabs4_uneven_mfma", SLABS4, 20, 12, True, "group", 4, 0, 3, (ROUTE_GRADW16, 4, 1, 2, 32, 1, 1, 1)),
    ("slabs4_uneven_fma", SLABS4, 5, 7, True, "shared", 1, 0, 3, (ROUTE_GRADW_FMA, 4, 0, 0, 32, 1, 1, 1)),
    ("kz2_oy2", (300, 0, 100), 272, 132, True, "group", 0, 0, 1, (ROUTE_GRADW16, 2, 4, 3, 6, 2, 2, 141)),
    ("k100_d100", (300, 0, 213), 100, 100, True, "shared", 4, 0, 1, (ROUTE_GRADW16, 2, 2, 4, 6, 1, 1, 40)),
    ("k68_d12", (300, 0, 213), 68, 12, True, "group", 0, 0, 1, (ROUTE_GRADW16, 2, 2, 3, 6, 1, 1, 4)),
    ("mfma_no_db", SIZES, 20, 12, True, None, 4, 0, 1, (ROUTE_GRADW16, 1, 1, 2, 12, 1, 1, 1)),
    ("db_only_wide", SIZES, 20, 300, False, "group", 0, 0, 1, (ROUTE_GRADW_FMA, 1, 0, 0, 12, 2, 1, 2)),
    ("fma_long_30x10", SIZES, 30, 10, True, "group", 1, 0, 1, (ROUTE_GRADW_FMA, 1, 0, 0, 12, 2, 1, 2)),
    # Dout * K + Dout = 252 at 20 x 12 is one pass of 256 lanes; 24 x 12 (300) is the misaligned shape with two
    ("fma_misaligned_20x12", SIZES, 20, 12, True, "shared", 4, 1, 1, (ROUTE_GRADW_FMA, 1, 0, 0, 12, 1, 1, 1)),
    ("fma_long_misaligned_24x12", SIZES, 24, 12, True, "shared", 4, 1, 1, (ROUTE_GRADW_FMA, 1, 0, 0, 12, 2, 1, 2)),
]


def forward64(x, W, seg, bias, relu, w_layout):
    # out [N, Dout] in float64: W [G, Dout, K] (w_layout 0) or [G, K, Dout] (1); bias None, [Dout] or [G, Dout]
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    out = np.zeros((x.shape[0], W.shape[1 if w_layout == 0 else 2]))
    for g in range(len(seg) - 1):
        r = slice(seg[g], seg[g + 1])
        out[r] = x[r] @ (W[g].T if w_layout == 0 else W[g])
        if bias is not None:
            out[r] += np.asarray(bias, np.float64).reshape(-1, out.shape[1])[g if np.ndim(bias) == 2 else 0]
    return np.maximum(out, 0.0) if relu else out


def grad64(dz, x, seg, shared_db=False):
    """(dW [G, Dout, K], db [G, Dout] or, shared, [Dout]) in float64"""
    dz, x = np.asarray(dz, np.float64), np.asarray(x, np.float64)
    G = len(seg) - 1
    dW = np.stack([dz[seg[g]:seg[g + 1]].T @ x[seg[g]:seg[g + 1]] for g in range(G)])
    db = np.stack([dz[seg[g]:seg[g + 1]].sum(0) for g in range(G)])
    return dW, (db.sum(0) if shared_db else db)


def build_forward(ctx):
    # (sizes, K, Dout, w_layout, bias, relu, tags): two MFMA shapes (K tail, partial column block; two column tiles), two of the any-shape kernel
    shapes = ((SIZES, 20, 12, 0, "group", 1, {"align", "side"}), (SIZES, 100, 132, 1, "shared", 0, ()), (SIZES, 5, 7, 1, None, 0, {"align"}),
              ((4, 0, 9), 2, 3, 0, "group", 1, ()))
    for sizes, K, Dout, lay, bias, relu, tags in shapes:
        seg = seg_of(sizes)
        N, G = int(seg[-1]), len(sizes)
        r = A.rng_of("grouped_dense", sizes, K, Dout, lay)
        x, W = A.F(r, N, K), A.F(r, G, *((Dout, K) if lay == 0 else (K, Dout)))
        b = None if bias is None else A.F(r, *((G, Dout) if bias == "group" else (Dout,)))
        job = A.Rec("gnnmp_grouped_dense_t", x=A.Arr("x", "in", x), ldx=K, W=A.Arr("W", "in", W), w_stride=Dout * K, ldw=K if lay == 0 else Dout,
                    w_layout=lay, bias=None if b is None else A.Arr("bias", "in", b), bias_stride=Dout if bias == "group" else 0,
                    seg_ptr=A.Arr("seg_ptr", "in", seg), act=relu, out=A.Arr("out", "out", shape=(N, Dout)), ldo=Dout)
        yield A.mk(FWD, f"G{G}_N{N}_K{K}_D{Dout}_l{lay}_b{bias}_a{relu}", tags, [job, N, G, K, Dout, A.STREAM],
                   lambda host, v=(x, W, seg, b, relu, lay): {"out": A.E(forward64(*v), "rel")})


def build_grad(ctx):
    # (sizes, K, Dout, dW?, db, tags): MFMA with one slab a group and, on two long groups, two; the any-shape kernel; db alone
    shapes = ((SIZES, 20, 12, True, "group", {"align", "side"}), ((300, 0, 213), 24, 100, True, "shared", ()), (SIZES, 5, 7, True, None, {"align"}),
              (SIZES, 4, 8, False, "group", ()))
    for sizes, K, Dout, want_w, db, tags in shapes:
        seg = seg_of(sizes)
        N, G = int(seg[-1]), len(sizes)
        r = A.rng_of("grouped_dense_grad", sizes, K, Dout)
        dz, x = A.F(r, N, Dout), A.F(r, N, K)
        floats = G * max(1, N // G // 64) * (Dout * K + Dout)        # the header's formula at its largest S: no more than 64 rows a slab
        job = A.Rec("gnnmp_grouped_dense_grad_t", dz=A.Arr("dz", "in", dz), lddz=Dout, x=A.Arr("x", "in", x), ldx=K,
                    seg_ptr=A.Arr("seg_ptr", "in", seg), dW=A.Arr("dW", "out", shape=(G, Dout, K)) if want_w else None, dw_stride=Dout * K,
                    db=None if db is None else A.Arr("db", "out", shape=(G, Dout) if db == "group" else (Dout,)),
                    db_stride=Dout if db == "group" else 0, workspace=A.Arr("workspace", "scratch", shape=(floats,)), workspace_floats=floats)

        def ref(host, v=(dz, x, seg, db == "shared"), want_w=want_w, db=db):
            dW, dbv = grad64(*v)
            return {**({"dW": A.E(dW, "rel")} if want_w else {}), **({"db": A.E(dbv, "rel")} if db else {})}
        yield A.mk(GRAD, f"G{G}_N{N}_K{K}_D{Dout}_w{int(want_w)}_b{db}", tags, [job, N, G, K, Dout, A.STREAM], ref)


for _name, _build in ((FWD, build_forward), (GRAD, build_grad)):
    A.TABLE.setdefault(_name, A._of_variant(_build))      # as the registry's last lines wrap every builder it holds
