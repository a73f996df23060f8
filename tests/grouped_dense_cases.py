"""The cases of the grouped dense exports (csrc/dense_grouped.hip) for the ABI's memory contract, beside tests/abi_cases.py as
tests/topk_cases.py is: importing this module registers both exports in TABLE (they only launch).  tests/test_grouped_dense_abi.py runs the
contract and capture checks over them; the float64 restatements, group by group, also serve tests/test_grouped_dense.py."""
import numpy as np

import abi_cases as A

FWD, GRAD = "gnnmp_grouped_dense_f32", "gnnmp_grouped_dense_grad_w_f32"
SIZES = (0, 1, 15, 16, 17, 0, 40, 3, 3, 3, 3, 70)      # empty groups in front and inside, a 16-row tile cut four times, a group over several tiles
seg_of = lambda sizes: np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)      # noqa: E731


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
