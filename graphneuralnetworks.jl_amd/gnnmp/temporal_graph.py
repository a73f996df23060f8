"""TemporalSnapshotsGNNGraph — GNNGraphs/src/temporalsnapshotsgnngraph.jl:56-231: a graph that changes from step to step, held as a list
of GNNGraph snapshots (their node and edge counts may differ).  add_snapshot / remove_snapshot (:132-145, :192-201) return new objects.

POSITIONS ARE PYTHON'S, 0-BASED: tg[0] is the reference's tg[1], add_snapshot(tg, 0, g) puts g in front (the reference's t = 1) and
add_snapshot(tg, len(tg), g) appends (the reference's t = num_snapshots + 1).

What the reference does not have: tg.batched() — the block-diagonal GNNGraph of the snapshots (gnnmp.batch) with their row offsets, built
on first use and kept; the snapshots are independent given their weights, so a layer can aggregate all of them in one launch
(gnnmp.EvolveGCNO).
"""
from __future__ import annotations

import torch

from .graph import GNNGraph, batch


def _same_graph(a, b):
    """the reference's == on two GNNGraph (field by field) for what a snapshot holds here: sizes, edge index, edge weights"""
    if a is b:
        return True
    if (a.num_nodes, a.num_edges, a.num_graphs, a.index_base) != (b.num_nodes, b.num_edges, b.num_graphs, b.index_base):
        return False
    if (a.w is None) != (b.w is None):
        return False
    return bool(torch.equal(a.s, b.s) and torch.equal(a.t, b.t) and (a.w is None or torch.equal(a.w, b.w)))


def _check_members(who, snapshots):
    for k, g in enumerate(snapshots):
        if not isinstance(g, GNNGraph):
            raise TypeError(f"{who}: snapshot {k} is a {type(g).__name__}, not a GNNGraph")
    devs = {str(g.device) for g in snapshots}
    if len(devs) > 1:
        raise ValueError(f"{who}: the snapshots are on different devices ({', '.join(sorted(devs))})")


class TemporalSnapshotsGNNGraph:
    """TemporalSnapshotsGNNGraph(snapshots) — temporalsnapshotsgnngraph.jl:56-73.  Fields as in the reference: num_nodes and num_edges
    (lists, one entry a snapshot), num_snapshots, snapshots, tgdata (a dict, carried along by indexing, add_snapshot and remove_snapshot).
    len(tg), iteration and tg[t] give snapshots; tg[list | slice] a new temporal graph; tg[t] = g replaces a snapshot; == compares
    snapshot by snapshot.  Positions are 0-based (the reference's are 1-based): tg[0] is the first snapshot."""

    def __init__(self, snapshots, tgdata=None):
        snapshots = list(snapshots)
        _check_members("TemporalSnapshotsGNNGraph", snapshots)
        self.snapshots = snapshots
        self.num_nodes = [g.num_nodes for g in snapshots]
        self.num_edges = [g.num_edges for g in snapshots]
        self.tgdata = {} if tgdata is None else tgdata
        self._batched = None

    @property
    def num_snapshots(self):
        return len(self.snapshots)

    @property
    def device(self):
        return self.snapshots[0].device if self.snapshots else None

    def __len__(self):
        return len(self.snapshots)

    def __iter__(self):
        return iter(self.snapshots)

    def _position(self, who, t, end):
        """a 0-based position in [0, end), negative ones counted from the end as Python does"""
        if isinstance(t, bool) or not isinstance(t, int):
            raise TypeError(f"{who}: a position is an int, got {type(t).__name__}")
        if not -end <= t < end:
            raise IndexError(f"{who}: position {t} is past the end, the temporal graph has {self.num_snapshots} snapshots "
                             f"(positions are 0-based)")
        return t % end if end else 0

    def __getitem__(self, t):
        if isinstance(t, slice):
            return TemporalSnapshotsGNNGraph(self.snapshots[t], self.tgdata)
        if isinstance(t, (list, tuple)):
            return TemporalSnapshotsGNNGraph([self.snapshots[self._position("TemporalSnapshotsGNNGraph", k, len(self))] for k in t],
                                             self.tgdata)
        return self.snapshots[self._position("TemporalSnapshotsGNNGraph", t, len(self))]

    def __setitem__(self, t, g):
        t = self._position("TemporalSnapshotsGNNGraph", t, len(self))
        _check_members("TemporalSnapshotsGNNGraph", self.snapshots[:t] + [g] + self.snapshots[t + 1:])
        self.snapshots[t] = g
        self.num_nodes[t] = g.num_nodes
        self.num_edges[t] = g.num_edges
        self._batched = None

    def __eq__(self, other):
        if self is other:
            return True
        if not isinstance(other, TemporalSnapshotsGNNGraph):
            return NotImplemented
        if (self.num_nodes, self.num_edges, self.tgdata) != (other.num_nodes, other.num_edges, other.tgdata):
            return False
        return all(_same_graph(a, b) for a, b in zip(self.snapshots, other.snapshots))

    __hash__ = None

    def batched(self):
        """(gb, seg_ptr): the block-diagonal GNNGraph of the snapshots (gnnmp.batch: snapshot t is the rows seg_ptr[t] .. seg_ptr[t + 1]
        of gb) and the T + 1 row offsets, a Python list.  Built on the first call and kept — its plans and normalisation caches with it;
        tg[t] = g drops it."""
        if self._batched is None:
            if not self.snapshots:
                raise ValueError("TemporalSnapshotsGNNGraph.batched: no snapshots")
            seg = [0]
            for n in self.num_nodes:
                seg.append(seg[-1] + n)
            gb = self.snapshots[0] if len(self.snapshots) == 1 else batch(self.snapshots)
            self._batched = (gb, seg)
        return self._batched

    def __repr__(self):
        return f"TemporalSnapshotsGNNGraph({self.num_snapshots})"


def add_snapshot(tg: TemporalSnapshotsGNNGraph, t: int, g: GNNGraph) -> TemporalSnapshotsGNNGraph:
    """add_snapshot(tg, t, g) — temporalsnapshotsgnngraph.jl:132-145: a NEW temporal graph with g at position t (0-based: 0 puts it in
    front, len(tg) appends; the reference's t is this t + 1); tg is left alone.  As in the reference, g must have the node count of tg's
    first snapshot."""
    if not isinstance(tg, TemporalSnapshotsGNNGraph):
        raise TypeError(f"add_snapshot: expected a TemporalSnapshotsGNNGraph, got {type(tg).__name__}")
    if not isinstance(g, GNNGraph):
        raise TypeError(f"add_snapshot: the snapshot is a {type(g).__name__}, not a GNNGraph")
    if isinstance(t, bool) or not isinstance(t, int) or not 0 <= t <= tg.num_snapshots:
        raise IndexError(f"add_snapshot: cannot add a snapshot at position {t}, the temporal graph has only {tg.num_snapshots} snapshots "
                         f"(positions are 0-based: 0 .. {tg.num_snapshots})")
    if tg.num_snapshots > 0 and g.num_nodes != tg.num_nodes[0]:
        raise ValueError(f"add_snapshot: number of nodes must match ({g.num_nodes} against {tg.num_nodes[0]})")
    snaps = list(tg.snapshots)
    snaps.insert(t, g)
    return TemporalSnapshotsGNNGraph(snaps, tg.tgdata)


def remove_snapshot(tg: TemporalSnapshotsGNNGraph, t: int) -> TemporalSnapshotsGNNGraph:
    """remove_snapshot(tg, t) — temporalsnapshotsgnngraph.jl:192-201: a NEW temporal graph without the snapshot at position t (0-based);
    tg is left alone"""
    if not isinstance(tg, TemporalSnapshotsGNNGraph):
        raise TypeError(f"remove_snapshot: expected a TemporalSnapshotsGNNGraph, got {type(tg).__name__}")
    if isinstance(t, bool) or not isinstance(t, int) or not 0 <= t < tg.num_snapshots:
        raise IndexError(f"remove_snapshot: position {t} is past the end, the temporal graph has {tg.num_snapshots} snapshots "
                         f"(positions are 0-based)")
    snaps = list(tg.snapshots)
    del snaps[t]
    return TemporalSnapshotsGNNGraph(snaps, tg.tgdata)
