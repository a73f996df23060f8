"""Heterograph attention at the layer level, on the GPU: gat_conv / gatv2_conv on a (x_src, x_dst) pair, HeteroGraphConv with GATConv /
GATv2Conv members (the fused launch of csrc/hetero_attn.hip against the per-member composition, the route asserted) and hetero_conv_ad,
all against the float64 restatement tests/hetero_attn_ref.py within the project's 1e-5 (abi_cases.compare).

The graph: A (9 nodes), B (13), C (5), D (4).  B receives from A, from C, from itself and from D (a relation without edges: D is a source
type with no out-edge); A receives from B.  B is both source and destination."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import hetero_attn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
NUM = {"A": 9, "B": 13, "C": 5, "D": 4}
ETS = [("A", "ab", "B"), ("C", "cb", "B"), ("B", "ba", "A"), ("B", "bb", "B"), ("D", "db", "B")]
EDGES = {ETS[0]: 40, ETS[1]: 17, ETS[2]: 30, ETS[3]: 25, ETS[4]: 0}
CIN, H, C = 5, 2, 4
KINDS = (0, 1, 1, 0, 0)      # R.GAT | R.GATV2 per relation: both kinds arrive at B; the relation of B onto itself and the empty one are GAT
FWD = ("gnnmp_hetero_attn_f32", "gnnmp_gat_conv_f32", "gnnmp_attn_conv_f32", "gnnmp_gat_conv_stats_f32", "gnnmp_dense_f32")


@pytest.fixture(scope="module")
def gm():
    import torch
    assert torch.cuda.is_available()
    import gnnmp
    return gnnmp


def close64(got, ref, what):
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    msg = A.compare(got, np.asarray(ref), A.E(tol="rel"))
    assert msg is None, f"{what}: {msg}"


def spy(monkeypatch, *names):
    from gnnmp import _lib
    lib = _lib.load()
    counts = {n: 0 for n in names}
    for n in names:
        real = getattr(lib, n)

        def wrapped(*a, _real=real, _n=n):
            counts[_n] += 1
            return _real(*a)
        monkeypatch.setattr(lib, n, wrapped)
    return counts


def graph(gm, seed=3, hub=False):
    rng = np.random.default_rng(seed)
    coo = {et: (rng.integers(0, NUM[et[0]], EDGES[et]), rng.integers(0, NUM[et[2]], EDGES[et])) for et in ETS}
    if hub:      # one row of B longer than the plans' smallest split threshold (GNNMP_MIN_LONG_ROW = 64)
        s, t = coo[ETS[0]]
        coo[ETS[0]] = (np.concatenate([s, rng.integers(0, NUM["A"], 70)]), np.concatenate([t, np.full(70, 6)]))
    g = gm.GNNHeteroGraph({et: (s + 1, t + 1) for et, (s, t) in coo.items()}, num_nodes=NUM)
    x = {k: rng.uniform(-1, 1, (n, CIN)).astype(np.float32) for k, n in NUM.items()}
    return g, coo, x


def cuda(x):
    import torch
    return {k: torch.from_numpy(v).cuda() for k, v in x.items()}


def make_layer(gm, kind, sigma=None, concat=True, seed=0, heads=H, out=C):
    """(layer with random biases, its float64 parameters for the reference)"""
    import torch
    gen = torch.Generator().manual_seed(1000 + seed)
    rnd = lambda n: (torch.rand(n, generator=gen) * 2 - 1).cuda()      # noqa: E731
    if kind == R.GAT:
        l = gm.GATConv((CIN, out), sigma, heads=heads, concat=concat, add_self_loops=False, seed=seed)
    else:
        l = gm.GATv2Conv((CIN, out), sigma, heads=heads, concat=concat, add_self_loops=False, seed=seed)
        l.dense_i_bias = rnd(heads * out)
    l.bias = rnd(heads * out if concat else out)
    return l


def params_of(l):
    n = lambda t: None if t is None else t.detach().cpu().numpy().astype(np.float64)      # noqa: E731
    if hasattr(l, "dense_x_weight"):
        return R.gat_params(n(l.dense_x_weight), n(l.a), n(l.bias), l.heads, l.sigma, bool(l.concat), l.negative_slope)
    return R.gatv2_params(n(l.dense_i_weight), n(l.dense_i_bias), n(l.dense_j_weight), n(l.a), n(l.bias), l.heads, l.sigma, bool(l.concat),
                          l.negative_slope)


# ---- the bipartite forwards ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("sigma", [None, "relu"])
@pytest.mark.parametrize("kind", [R.GAT, R.GATV2])
def test_layer_on_a_pair_matches_the_reference(gm, kind, sigma, concat):
    g, coo, x = graph(gm)
    xd = cuda(x)
    for k, et in enumerate(ETS[:2] + ETS[3:]):      # bipartite, bipartite, a type onto itself, a relation without edges
        l = make_layer(gm, kind, sigma, concat, seed=10 + k)
        y = l(gm.edge_type_subgraph(g, et), (xd[et[0]], xd[et[2]]))
        assert y.shape == (NUM[et[2]], H * C if concat else C)
        close64(y, R.layer_forward(params_of(l), *coo[et], NUM[et[2]], x[et[0]], x[et[2]]), f"{et}")


def test_a_pair_refuses_by_name_what_it_does_not_take(gm):
    import torch
    from gnnmp.layers import gat_conv
    g, coo, x = graph(gm)
    xd = cuda(x)
    et = ETS[0]
    rel, pair = gm.edge_type_subgraph(g, et), (xd["A"], xd["B"])
    e = torch.rand((EDGES[et], 3), device="cuda")
    for make, name in ((gm.GATConv, "GATConv"), (gm.GATv2Conv, "GATv2Conv")):
        with pytest.raises(NotImplementedError, match=f"{name} on a .* pair: edge features"):
            make(((CIN, 3), C), heads=H, add_self_loops=False)(rel, pair, e)
        with pytest.raises(NotImplementedError, match=f"{name} on a .* pair: edge features"):
            make((CIN, C), heads=H, add_self_loops=False)(rel, pair, e)
        with pytest.raises(NotImplementedError, match=f"{name} on a .* pair: attention dropout"):
            make((CIN, C), heads=H, add_self_loops=False, dropout=0.3)(rel, pair)
        with pytest.raises(NotImplementedError, match=f"{name} on a .* pair: add_self_loops on a heterograph relation is out of scope"):
            make((CIN, C), heads=H)(rel, pair)
    l = gm.GATConv((CIN, C), heads=H, add_self_loops=False)
    for kw in (dict(return_alpha=True), dict(exact_order=True)):
        with pytest.raises(NotImplementedError, match="GATConv on a .* pair: return_alpha / exact_order"):
            gat_conv(l, rel, pair, **kw)


# ---- HeteroGraphConv -------------------------------------------------------------------------------------------------------------------
def model_of(gm, sigma, aggr, concat_b=True, seed=20):
    layers = {et: make_layer(gm, KINDS[k], sigma, concat_b if et[2] == "B" and k == 1 else True, seed=seed + k)
              for k, et in enumerate(ETS)}
    return gm.HeteroGraphConv(layers, aggr=aggr)


def ref_of(model, coo, x):
    members = [(et, params_of(l)) for et, l in zip(model.etypes, model.layers)]
    return R.conv_forward(members, coo, NUM, x, model.aggr)


@pytest.mark.parametrize("sigma", [None, "relu"])
@pytest.mark.parametrize("aggr", ["+", "max", "min"])
def test_fused_path_and_composition_agree_and_match_the_reference(gm, monkeypatch, aggr, sigma):
    from gnnmp import _lib
    g, coo, x = graph(gm)
    model = model_of(gm, sigma, aggr)
    counts = spy(monkeypatch, *FWD)
    y = model(g, cuda(x))
    assert counts["gnnmp_hetero_attn_f32"] == 1 and counts["gnnmp_gat_conv_f32"] == counts["gnnmp_attn_conv_f32"] == 0      # B and A: one launch
    with _lib.tuned(_lib.Knob.HETERO, -1):
        yc = model(g, cuda(x))
    assert counts["gnnmp_hetero_attn_f32"] == 1 and counts["gnnmp_gat_conv_f32"] + counts["gnnmp_attn_conv_f32"] == len(ETS)
    ref = ref_of(model, coo, x)
    assert list(y) == list(yc) == ["B", "A"]
    for k in y:
        close64(y[k], ref[k], f"fused {k}")
        close64(yc[k], ref[k], f"composition {k}")
        close64(y[k], yc[k].cpu().numpy().astype(np.float64), f"fused vs composition {k}")


def test_the_fused_path_is_not_taken_where_it_is_not_eligible(gm, monkeypatch):
    g, coo, x = graph(gm)
    counts = spy(monkeypatch, *FWD)
    # concat = false members at B (heads averaged: out = C wide) beside one concat = true member of the same width (heads * out = C)
    layers = {et: make_layer(gm, KINDS[k], "relu", concat=et[2] != "B", seed=40 + k, out=C if et[2] == "B" else C // H)
              for k, et in enumerate(ETS)}
    layers[ETS[0]] = make_layer(gm, R.GAT, "relu", concat=True, seed=39, out=C // H)
    model = gm.HeteroGraphConv(layers, aggr="+")
    y = model(g, cuda(x))
    assert counts["gnnmp_hetero_attn_f32"] == 1                                            # A alone
    assert counts["gnnmp_gat_conv_f32"] + counts["gnnmp_attn_conv_f32"] == 4              # B by its members
    ref = ref_of(model, coo, x)
    for k in y:
        close64(y[k], ref[k], f"concat = false at B: {k}")
    # a GraphConv member beside an attention member at B
    for k in counts:
        counts[k] = 0
    gat, gc = make_layer(gm, R.GAT, None, seed=50), gm.GraphConv((CIN, H * C), seed=51)
    model = gm.HeteroGraphConv({ETS[0]: gat, ETS[1]: gc}, aggr="+")
    xd = cuda(x)
    y = model(g, xd)
    assert counts["gnnmp_hetero_attn_f32"] == 0 and counts["gnnmp_gat_conv_f32"] == 1
    want = gat(gm.edge_type_subgraph(g, ETS[0]), (xd["A"], xd["B"])) + gc(gm.edge_type_subgraph(g, ETS[1]), (xd["C"], xd["B"]))
    close64(y["B"], want.cpu().numpy().astype(np.float64), "mixed destination type")
    # a plan with split rows
    for k in counts:
        counts[k] = 0
    gh, cooh, xh = graph(gm, hub=True)
    assert gh.plan(ETS[0]).n_long > 0
    model = model_of(gm, None, "+")
    y = model(gh, cuda(xh))
    assert counts["gnnmp_hetero_attn_f32"] == 1 and counts["gnnmp_gat_conv_f32"] + counts["gnnmp_attn_conv_f32"] == 4      # A fused, B by its members
    ref = ref_of(model, cooh, xh)
    for k in y:
        close64(y[k], ref[k], f"split rows: {k}")


def test_a_shared_destination_projection_is_computed_once(gm, monkeypatch):
    g, coo, x = graph(gm)
    shared = make_layer(gm, R.GAT, None, seed=60)
    v2 = make_layer(gm, R.GATV2, None, seed=61)
    model = gm.HeteroGraphConv({ETS[0]: shared, ETS[1]: shared, ETS[3]: shared, ETS[4]: v2}, aggr="+")
    counts = spy(monkeypatch, *FWD)
    y = model(g, cuda(x))
    # dense_x of A, C and B once each (B's serves three relations as Q and one as K), dense_i of B and dense_j of D
    assert counts["gnnmp_hetero_attn_f32"] == 1 and counts["gnnmp_dense_f32"] == 5
    close64(y["B"], ref_of(model, coo, x)["B"], "shared projections")


# ---- training --------------------------------------------------------------------------------------------------------------------------
GRAD_NAMES = {R.GAT: (("dense_x_weight", "W"), ("a", "a"), ("bias", "bias")),
              R.GATV2: (("dense_i_weight", "Wi"), ("dense_i_bias", "bi"), ("dense_j_weight", "Wj"), ("a", "a"), ("bias", "bias"))}


@pytest.mark.parametrize("aggr,sigma,concat", [("+", None, True), ("max", "relu", True), ("+", "relu", False)])
def test_hetero_conv_ad_gradients_match_the_reference(gm, monkeypatch, aggr, sigma, concat):
    import torch
    g, coo, x = graph(gm, seed=5)
    layers = {et: make_layer(gm, KINDS[k], sigma, concat, seed=70 + k) for k, et in enumerate(ETS)}
    model = gm.HeteroGraphConv(layers, aggr=aggr)
    rng = np.random.default_rng(8)
    width = H * C if concat else C
    dout = {k: rng.uniform(-1, 1, (NUM[k], width)).astype(np.float32) for k in ("B", "A")}
    xd = {k: v.requires_grad_() for k, v in cuda(x).items()}
    leaves, names = [], []
    for et, l in zip(model.etypes, model.layers):
        for attr, ref_name in GRAD_NAMES[R.GAT if hasattr(l, "dense_x_weight") else R.GATV2]:
            leaves.append(getattr(l, attr).requires_grad_())
            names.append((et, ref_name))
    counts = spy(monkeypatch, *FWD)
    y = gm.hetero_conv_ad(model, g, xd)
    fused = aggr == "+" and sigma is None and concat
    assert counts["gnnmp_hetero_attn_f32"] == (1 if fused else 0)
    assert (counts["gnnmp_gat_conv_stats_f32"] + counts["gnnmp_attn_conv_f32"] == 0) == fused
    members = [(et, params_of(l)) for et, l in zip(model.etypes, model.layers)]
    ref = R.conv_forward(members, coo, NUM, x, aggr)
    for k in y:
        close64(y[k], ref[k], f"forward {k}")
    loss = sum((y[k] * torch.from_numpy(dout[k]).cuda()).sum() for k in y)
    grads = torch.autograd.grad(loss, list(xd.values()) + leaves)
    dx, gparams = R.conv_grad(members, coo, NUM, x, dout, aggr)
    for k, gk in zip(xd, grads):
        close64(gk, dx[k], f"Δx[{k}]")
    assert not dx["D"].any() and not grads[list(xd).index("D")].cpu().numpy().any()      # a source type with no out-edge: zeros, written
    by_et = {et: gp for (et, _), gp in zip(members, gparams)}
    for (et, ref_name), gk in zip(names, grads[len(xd):]):
        close64(gk, by_et[et][ref_name], f"Δ{ref_name} {et}")
    again = torch.autograd.grad(sum((v * torch.from_numpy(dout[k]).cuda()).sum() for k, v in gm.hetero_conv_ad(model, g, xd).items()),
                                list(xd.values()) + leaves)
    for a, b in zip(grads, again):
        assert torch.equal(a, b), "two calls give other bits"


def test_hetero_conv_ad_refuses_a_layer_that_mixes_member_kinds(gm):
    g, coo, x = graph(gm)
    model = gm.HeteroGraphConv({ETS[0]: make_layer(gm, R.GAT, seed=80), ETS[1]: gm.GraphConv((CIN, H * C), seed=81)})
    with pytest.raises(NotImplementedError, match="mixes attention members with GraphConv / SAGEConv members.*GATConv, GraphConv"):
        gm.hetero_conv_ad(model, g, cuda(x))
    assert model(g, cuda(x))["B"].shape == (NUM["B"], H * C)      # the forward runs, through the composition


def test_one_sgd_step_lowers_the_loss(gm):
    """HeteroGraphConv of GATConv -> relu -> HeteroGraphConv of GATv2Conv on a three-type graph, sum of squares loss"""
    import torch
    ets = ETS[:4]
    g, coo, x = graph(gm, seed=9)
    l1 = gm.HeteroGraphConv({et: make_layer(gm, R.GAT, "relu", seed=90 + k) for k, et in enumerate(ets)})
    ets2 = [et for et in ets if et[0] != "C"]      # A and B carry the hidden width; C only feeds the first layer
    l2 = gm.HeteroGraphConv({et: gm.GATv2Conv((H * C, C), heads=H, add_self_loops=False, seed=95 + k) for k, et in enumerate(ets2)})
    params = [p.requires_grad_() for m in (l1, l2) for l in m.layers
              for p in (([l.dense_x_weight, l.a, l.bias]) if hasattr(l, "dense_x_weight") else [l.dense_i_weight, l.dense_i_bias, l.dense_j_weight, l.a, l.bias])]
    xd = cuda(x)

    def loss():
        h = gm.hetero_conv_ad(l1, g, dict(xd))
        y = gm.hetero_conv_ad(l2, g, h)
        return sum((v * v).sum() for v in y.values())
    before = loss()
    grads = torch.autograd.grad(before, params)
    assert all(torch.isfinite(gk).all() for gk in grads) and any(gk.abs().max() > 0 for gk in grads)
    with torch.no_grad():
        for p, gk in zip(params, grads):
            p -= 1e-4 * gk
    after = loss()
    assert float(after) < float(before), (float(before), float(after))
