"""Float64 restatement of GATConv with edge features (GNNlib/src/layers/conv.jl:112-167, e !== nothing) and of every gradient of it, as
include/gnnmp.h states them for gnnmp_gat_conv_edge_stats_f32 / gnnmp_gat_conv_edge_grad_f32 / gnnmp_gat_edge_fold_f32 / _fold_grad_f32.
Plain numpy on the edge list, bipartite relations included (Wx_dst given).  tests/test_gat_edge_grad_ref.py pins the gradients by
central differences and the forward by the oracle; the GPU tests compare the kernels with this module.

Per head h, for edge k = (j -> i) at position k:
    z_ij = a_d . Wx_dst_i + a_s . Wx_src_j + es_k      l = leakyrelu(z)      α = softmax over the in-edges of i      o_i = Σ_j α_ij Wx_src_j
    g_ij = Δ_i . Wx_src_j    D_i = Σ_j α_ij g_ij    dz_ij = α_ij (g_ij - D_i) leakyrelu'(z_ij)    dsd_i = Σ_j dz_ij    dss_j = Σ_i dz_ij    des_k = dz_ij
    dWx_src_j = Σ_i α_ij Δ_i + a_s dss_j      dWx_dst_i = a_d dsd_i      da_d = Σ_i dsd_i Wx_dst_i      da_s = Σ_j dss_j Wx_src_j
and the edge side through M[h] = Σ_c a_e[h][c] W_e[hC + c]:  es = e M',  de = des M,  dM = des' e,  dW_e[hC + c] = a_e[h][c] dM[h],
da_e[h][c] = dM[h] . W_e[hC + c]."""
import numpy as np

f64 = np.float64


def seg_sum(idx, vals, n):
    out = np.zeros((n,) + vals.shape[1:], f64)
    np.add.at(out, idx, vals)
    return out


def lrelu(x, slope):
    return np.where(x > 0, x, slope * x)


def core(s, t, n_src, n_dst, Wx_src, Wx_dst, a, es, slope):
    """(o [n_dst][H][C], cache).  s, t: 0-based; Wx_src [n_src][H][C]; Wx_dst [n_dst][H][C] or None (= Wx_src, a square relation);
    a [H][2C] (targets first); es [E][H].  A row without in-edges: o = 0, m = -Inf, den = 0"""
    Wx_src, a, es = np.asarray(Wx_src, f64), np.asarray(a, f64), np.asarray(es, f64)
    Wd = Wx_src if Wx_dst is None else np.asarray(Wx_dst, f64)
    C = Wx_src.shape[2]
    z = (a[None, :, :C] * Wd[t]).sum(-1) + (a[None, :, C:] * Wx_src[s]).sum(-1) + es.reshape(len(s), a.shape[0])
    l = lrelu(z, slope)
    m = np.full((n_dst, a.shape[0]), -np.inf)
    np.maximum.at(m, t, l)
    ex = np.exp(l - m[t])
    den = seg_sum(t, ex, n_dst)
    al = ex / den[t]
    o = seg_sum(t, al[..., None] * Wx_src[s], n_dst)
    return o, dict(z=z, al=al, m=m, den=den, Wd=Wd)


def core_grad(s, t, n_src, n_dst, Wx_src, Wx_dst, a, es, slope, c, do):
    """every gradient of Σ do . o; do [n_dst][H][C].  With Wx_dst None the target term lands in dWx_src and dWx_dst is None"""
    Wx_src, a, do = np.asarray(Wx_src, f64), np.asarray(a, f64), np.asarray(do, f64)
    C = Wx_src.shape[2]
    al, z, Wd = c["al"], c["z"], c["Wd"]
    g = (do[t] * Wx_src[s]).sum(-1)
    D = seg_sum(t, al * g, n_dst)
    dz = al * (g - D[t]) * np.where(z > 0, 1.0, slope)
    dsd, dss = seg_sum(t, dz, n_dst), seg_sum(s, dz, n_src)
    dsrc = seg_sum(s, al[..., None] * do[t], n_src) + dss[..., None] * a[None, :, C:]
    ddst = dsd[..., None] * a[None, :, :C]
    da = np.concatenate([(dsd[..., None] * Wd).sum(0), (dss[..., None] * Wx_src).sum(0)], -1)
    out = dict(dsd=dsd, dss=dss, da=da, des=dz, D=D, g=g)
    if Wx_dst is None:
        out.update(dWx_src=dsrc + ddst, dWx_dst=None)
    else:
        out.update(dWx_src=dsrc, dWx_dst=ddst)
    return out


def fold(a_e, W_e):
    """M [H][ein] from a_e [H][C] and W_e [H*C][ein]"""
    a_e, W_e = np.asarray(a_e, f64), np.asarray(W_e, f64)
    H, C = a_e.shape
    return (a_e[..., None] * W_e.reshape(H, C, -1)).sum(1)


def fold_grad(a_e, W_e, dM):
    """(dW_e [H*C][ein], da_e [H][C])"""
    a_e, W_e, dM = np.asarray(a_e, f64), np.asarray(W_e, f64), np.asarray(dM, f64)
    H, C = a_e.shape
    dW = a_e[..., None] * dM[:, None, :]
    return dW.reshape(H * C, -1), (dM[:, None, :] * W_e.reshape(H, C, -1)).sum(-1)


def _act(sigma, v):
    return np.maximum(v, 0.0) if sigma == "relu" else v


def layer(s, t, n, x, e, W, We, a, bias, sigma, H, concat, slope=0.2):
    """the layer: x [n][Din], e [E][ein], W [H*C][Din], We [H*C][ein], a (3C, H) as the layer holds it, bias [H*C] | [C] | None.
    Returns (y, cache)"""
    x, e, W, We, a = (np.asarray(v, f64) for v in (x, e, W, We, a))
    C = W.shape[0] // H
    at = a.T
    Wx = (x @ W.T).reshape(n, H, C)
    M = fold(at[:, 2 * C:], We)
    es = e @ M.T
    o, c = core(s, t, n, n, Wx, None, at[:, :2 * C], es, slope)
    pre = o.reshape(n, H * C) if concat else o.mean(1)
    pre = pre + (0.0 if bias is None else np.asarray(bias, f64))
    c.update(Wx=Wx, M=M, es=es, pre=pre, at=at)
    return _act(sigma, pre), c


def layer_grad(s, t, n, x, e, W, We, a, bias, sigma, H, concat, c, dy, slope=0.2):
    """dict(dx, de, dW, dWe, da (3C, H), db) of Σ dy . y"""
    x, e, W, We, dy = (np.asarray(v, f64) for v in (x, e, W, We, dy))
    C = W.shape[0] // H
    at = c["at"]
    dpre = dy * (c["pre"] > 0) if sigma == "relu" else dy
    do = dpre.reshape(n, H, C) if concat else np.repeat(dpre[:, None, :] / H, H, 1)
    gr = core_grad(s, t, n, n, c["Wx"], None, at[:, :2 * C], c["es"], slope, c, do)
    dWx = gr["dWx_src"].reshape(n, H * C)
    des = gr["des"]
    dM = des.T @ e
    dWe, da_e = fold_grad(at[:, 2 * C:], We, dM)
    return dict(dx=dWx @ W, dW=dWx.T @ x, de=des @ c["M"], dWe=dWe, da=np.concatenate([gr["da"], da_e], 1).T,
                db=None if bias is None else dpre.sum(0), des=des)
