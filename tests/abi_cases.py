"""Helpers of tests/test_abi_memory_contract.py: the header parser, the guarded slab every device array of a call is carved from, and the
case table over the C ABI (one builder per export: its arguments at a given shape, the role of every array, the float64 / exact reference).

Everything here calls libgnnmp.so through ctypes with raw pointers INTO the slab — never through the Python wrappers, which allocate
their own outputs.  Plans and the chain's job handles (opaque, library-owned) are the only objects created outside the slab.

TABLE holds the exports that only launch on their stream (and the graph prep the capture test quotes as exempt); PREP_TABLE the plan
writers and gnnmp_chain_jobs_export, which synchronise: the same cases and the same slab, never recorded into a HIP graph."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gnnmp.h")

OK, EINVAL, EBOUNDS, EUNSUPPORTED = 0, -1, -2, -5
SUM, MEAN, MAX, MIN = 0, 1, 2, 3
SPLIT_BOUND = 6e-7      # tests/test_dense_split.py: error of the split-bf16 dense core relative to sum_k |w_k x_k|
RTOL = 1e-5             # the parity tests' bound, relative to the reference's scale
RTOL64 = 1e-12          # the same for the Float64 entry points (tests/test_float64.py)


# ------------------------------------------------------------------------------------------------------------------------------------
# include/gnnmp.h
# ------------------------------------------------------------------------------------------------------------------------------------
HANDLE_TYPES = ("gnnmp_graph_t", "gnnmp_arena_t", "gnnmp_chain_jobs_t")
# pointer parameters the header documents as HOST memory (results of calls that synchronise, host tables of device pointers)
HOST_PARAMS = {"result", "result_host", "total", "n_new", "cls", "info", "ptr"}
# const HOST arrays of scalars, per export (the header: "dims : HOST int64 [n_layers + 1]", "act : HOST int [n_layers]")
HOST_ARRAYS = {"gnnmp_graphconv_chain_f32": ("dims", "act")}


RECORD_TYPE = re.compile(r"\bgnnmp_\w+_t\b")


class Header(tuple):
    """(decls, defines) as it always unpacked, with the header's records on the side: .records = {gnnmp_<x>_t: [(name, is_pointer,
    is_const, type text)]}, the fields of every `typedef struct { ... } gnnmp_<x>_t;` in declaration order"""
    records = {}


def _fields(body):
    """the fields of one struct body: `const float *fs_i, *fs_j;` and `float alpha, beta;` are one field a declarator"""
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        first, *more = [d.strip() for d in decl.split(",")]
        m = re.match(r"(.*?)(\**)\s*(\w+)$", first)
        base, stars, fname = m.group(1).strip(), m.group(2), m.group(3)
        out.append((fname, bool(stars), base.startswith("const"), f"{base} {stars}{fname}"))
        for d in more:
            m = re.match(r"(\**)\s*(\w+)$", d)
            out.append((m.group(2), bool(m.group(1)), base.startswith("const"), f"{base} {m.group(1)}{m.group(2)}"))
    return out


def parse_header(path=HEADER):
    """{export: [(name, is_pointer, is_const, type text)]} for every function the header declares, and its #define constants; the
    result's .records holds the fields of every record type the same way"""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    defines = {m.group(1): m.group(2) for m in re.finditer(r"#define\s+(GNNMP_\w+)\s+(-?\d+)", text)}
    decls = {}
    for m in re.finditer(r"\b(?:int64_t|int|void \*|const char \*)\s*(gnnmp_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        name, params = m.group(1), " ".join(m.group(2).split())
        out = []
        if params != "void":
            for p in params.split(","):
                p = p.strip()
                pname = re.search(r"(\w+)\s*(?:\[\d*\])?$", p).group(1)
                is_ptr = "*" in p or "[" in p
                out.append((pname, is_ptr, p.startswith("const"), p))
        decls[name] = out
    h = Header((decls, defines))
    h.records = {m.group(2): _fields(m.group(1)) for m in re.finditer(r"typedef struct\s*\{(.*?)\}\s*(gnnmp_\w+_t)\s*;", text, flags=re.S)}
    return h


def record_of(text, records):
    """the record type a parameter or field of type `text` points at, or None"""
    for t in RECORD_TYPE.findall(text):
        if t in records:
            return t
    return None


def is_host_param(export, pname):
    return pname in HOST_PARAMS


def device_pointer_params(export, decl):
    """[(name, is_const)] of the parameters that are device arrays (not handles, not the stream, not documented host memory)"""
    out = []
    for pname, is_ptr, is_const, text in decl:
        if not is_ptr or any(h in text for h in HANDLE_TYPES) or is_host_param(export, pname):
            continue
        out.append((pname, is_const))
    return out


def record_device_fields(export, rtype, records, seen=()):
    """[(record type, field, is_const)] of the device-pointer fields a record parameter hands over, nested tables followed (a field that
    points at another record — the hetero destination's `rels` — is that record's fields, not an array itself)"""
    out = []
    for fname, is_ptr, is_const, text in records[rtype]:
        if not is_ptr or any(h in text for h in HANDLE_TYPES) or is_host_param(export, fname):
            continue
        inner = record_of(text, records)
        if inner is not None:
            if inner not in seen:
                out += record_device_fields(export, inner, records, seen + (rtype,))
            continue
        out.append((rtype, fname, is_const))
    return out


def writes_of(export, decl, records):
    """how an export writes device memory: ([non-const pointer parameters], [(record type, non-const pointer field)])"""
    direct = [n for n, c in device_pointer_params(export, decl) if not c and record_of(dict((p[0], p[3]) for p in decl)[n], records) is None]
    through = []
    for pname, is_ptr, is_const, text in decl:
        rtype = record_of(text, records) if is_ptr else None
        if rtype is not None:
            through += [(rt, f) for rt, f, c in record_device_fields(export, rtype, records) if not c]
    return direct, through


def must_be_covered(decls, symbols, records=None, why=None):
    """the exports the case table owes: in SYMBOLS, take a stream, and write through a device pointer — a non-const pointer parameter, or
    a non-const pointer field of a record parameter (`const gnnmp_<x>_t *job` is a const HOST record: what it points at is written).
    records: parse_header().records — the completeness guard passes them; WITHOUT them only the parameters are looked at, which is what
    the per-family tests mean when they assert that an export "takes const host records" (no device pointer among its parameters).
    why: a dict that receives {export: 'param' | 'record'}, the first reason an export is owed for"""
    records = {} if records is None else records
    need = []
    for name in symbols:
        decl = decls.get(name)
        if not decl or not any("gnnmp_stream_t" in p[3] for p in decl):
            continue
        direct, through = writes_of(name, decl, records)
        if direct or through:
            need.append(name)
            if why is not None:
                why[name] = "param" if direct else "record"
    return need


# ------------------------------------------------------------------------------------------------------------------------------------
# the slab
# ------------------------------------------------------------------------------------------------------------------------------------
# 8 bytes, little endian: the float32 at an even word is the quiet NaN 0x7fc0beef, at an odd word 0x7ff8beef, the float64 at any 8-byte
# offset 0x7ff8beef7fc0beef (quiet NaN) — fixed payloads; read as integers every word is odd and far outside any index the tests use
PATTERN = np.frombuffer((0x7ff8beef7fc0beef).to_bytes(8, "little"), np.uint8)
GUARD_MIN = 4096
# shifts of an array's start, in bytes: 16-byte aligned but not 128, 8 but not 16, 4 only (taken in whole elements: a shift smaller than
# the element is skipped for that array)
SHIFTS = {"a16": 16, "a8": 8, "a4": 4}


class Arr:
    """one device array of a call.  role: 'in' (const T *: must come back bit for bit), 'out' (every element written), 'inout'
    (initialised by the caller, then compared), 'scratch' (caller-supplied work space: only its guards are checked)"""

    def __init__(self, name, role, data=None, shape=None, dtype=np.float32, field=None, base=None, offset=0):
        """field: the header's name of the parameter / record field when `name` (the slab's key, unique within a call) is another.
        base, offset: a VIEW — this argument is the pointer `offset` elements into the array `base` (a column block of a panel, a second
        name for one buffer); it owns no bytes of the slab, its role is what the header says of the field it is passed as, and what may
        be written where is stated by the role and the reference of the base.  Row strides are scalar fields of the record"""
        assert role in ("in", "out", "inout", "scratch")
        self.name, self.role, self.field, self.base, self.offset = name, role, field or name, base, int(offset)
        if base is not None:
            assert data is None and base.base is None and 0 <= self.offset <= max(int(np.prod(base.shape, dtype=np.int64)), 0)
            assert role == "in" or base.role != "in", f"'{name}' is written through, its base '{base.name}' is an input"
            self.data, self.shape, self.dtype, self.nbytes, self.off = None, (), base.dtype, 0, None
            return
        if data is not None:
            self.data = np.ascontiguousarray(data)
            self.shape, self.dtype = self.data.shape, self.data.dtype
        else:
            assert role in ("out", "scratch")
            self.data = None
            self.shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list)) else (shape,)))
            self.dtype = np.dtype(dtype)
        self.dtype = np.dtype(self.dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.off = None


class E:
    """what the reference says about one output.  value: the expected array (compared over its own length: `prefix` outputs are longer
    buffers of which only the first len(value) / prefix elements are owed); tol: 'exact' | 'rel' | 'mag' (mag: |err| <= SPLIT_BOUND * mag,
    and 'rel'); exact_rows: boolean row mask that must be bit-equal even when tol is 'rel'; pred(got) -> None | message"""

    def __init__(self, value=None, tol="rel", prefix=None, pred=None, exact_rows=None, mag=None, rows=None, scale=0.0):
        self.value, self.tol, self.prefix, self.pred, self.exact_rows, self.mag = value, tol, prefix, pred, exact_rows, mag
        # scale: a floor for "the reference's scale" where the reference is a DIFFERENCE of float64 terms that may cancel to exactly zero
        # (the softmax pullback's α (g - Σ α g) on a one-edge row): rounding error lives on the scale of the terms, and the case states it
        self.scale = scale                         # a float, or one floor per row of the output
        self.rows = rows      # boolean row mask: only these rows are compared (every element must still have been written)


def _round_up(v, m):
    return (v + m - 1) // m * m


class Slab:
    def __init__(self, arrs, device="cuda", shifts=None, guard=GUARD_MIN):
        import torch
        shifts = shifts or {}
        guard = _round_up(max(GUARD_MIN, int(guard)), 256)
        self.arrs = {}
        off = 0
        for a in arrs:
            assert a.name not in self.arrs, a.name
            sh = int(shifts.get(a.name, 0))
            assert sh % a.dtype.itemsize == 0, "shifts are whole elements"
            off += guard
            a.off = off + sh
            off = _round_up(a.off + a.nbytes, 256)
            self.arrs[a.name] = a
        self.total = off + guard
        self.pattern = np.tile(PATTERN, self.total // 8)
        host = self.pattern.copy()
        for a in arrs:
            if a.role in ("in", "inout"):
                host[a.off:a.off + a.nbytes] = a.data.reshape(-1).view(np.uint8)
        self.before = host
        self.t = torch.from_numpy(host.copy()).to(device)
        assert self.t.data_ptr() % 256 == 0 or device == "cpu"

    def ptr(self, name):
        return ctypes.c_void_p(self.t.data_ptr() + self.arrs[name].off)

    def ptr_of(self, a):
        """the pointer of an argument: an array of the slab, or a view `offset` elements into one"""
        if a.base is None:
            return self.ptr(a.name)
        return ctypes.c_void_p(self.t.data_ptr() + self.arrs[a.base.name].off + a.offset * a.base.dtype.itemsize)

    def reload(self, inputs=None):
        """the slab as before a call, at the SAME device addresses: poison in every output, scratch array and guard band, the initial
        data in every in / inout array.  inputs: {name: array} replaces the data of those in / inout arrays (same shape and type)"""
        import torch
        host = self.before.copy()
        for name, data in (inputs or {}).items():
            a = self.arrs[name]
            data = np.ascontiguousarray(data)
            assert a.role in ("in", "inout") and data.shape == a.shape and data.dtype == a.dtype, name
            host[a.off:a.off + a.nbytes] = data.reshape(-1).view(np.uint8)
        self.before = host
        self.t.copy_(torch.from_numpy(host.copy()))

    def outputs(self):
        """the bytes of every out / inout array as they are on the device now"""
        after = self.t.cpu().numpy()
        return {a.name: after[a.off:a.off + a.nbytes].copy() for a in self.arrs.values() if a.role in ("out", "inout")}

    def _where(self, byte):
        best = None
        for a in self.arrs.values():
            if a.off <= byte < a.off + max(a.nbytes, 1):
                return f"inside {a.role} array '{a.name}' (element {(byte - a.off) // a.dtype.itemsize})"
            d = byte - (a.off + a.nbytes) if byte >= a.off + a.nbytes else a.off - byte
            side = "after" if byte >= a.off + a.nbytes else "before"
            if best is None or d < best[0]:
                best = (d, f"{d} bytes {side} array '{a.name}'" if side == "before" else f"{d} bytes past the end of array '{a.name}'")
        return "in a guard band, " + best[1]

    def get(self, after, name):
        a = self.arrs[name]
        return after[a.off:a.off + a.nbytes].view(a.dtype).reshape(a.shape)

    def check(self, expected, untouched=False):
        """problems (list of strings) after the call.  expected: {name: E | ndarray}.  untouched: the call refused with a status —
        nothing at all may have been written"""
        after = self.t.cpu().numpy()
        problems = []
        owned = np.zeros(self.total, bool)
        if not untouched:
            for a in self.arrs.values():
                if a.role != "in":
                    owned[a.off:a.off + a.nbytes] = True
        bad = np.flatnonzero((after != self.before) & ~owned)
        if bad.size:                                # one problem per place: an input array, or the band between two arrays
            cuts = sorted({0, self.total} | {a.off for a in self.arrs.values()} | {a.off + a.nbytes for a in self.arrs.values()})
            for lo, hi in zip(cuts, cuts[1:]):
                here = bad[(bad >= lo) & (bad < hi)]
                if here.size:
                    problems.append(f"{here.size} stray byte(s) written, first {self._where(int(here[0]))}"
                                    + (" (the call returned an error status)" if untouched else ""))
        if untouched:
            return problems
        for name, exp in expected.items():
            a = self.arrs[name]
            if not isinstance(exp, E):
                exp = E(exp, tol="rel")
            got = self.get(after, name)
            flat = got.reshape(-1)
            if exp.prefix is not None:
                flat = flat[:int(exp.prefix)]
            elif exp.value is not None:
                v = np.asarray(exp.value)
                assert v.size == flat.size, f"{name}: reference has {v.size} elements, the buffer {flat.size}"
            if a.role == "out":
                u = {1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
                pat = self.pattern[a.off:a.off + flat.size * a.dtype.itemsize].view(u)
                unwritten = np.flatnonzero(flat.view(u) == pat)
                if unwritten.size:
                    problems.append(f"output '{name}': {unwritten.size} of {flat.size} element(s) never written, first at element {int(unwritten[0])}")
                    continue
            if exp.pred is not None:
                msg = exp.pred(flat if exp.prefix is not None else got)
                if msg:
                    problems.append(f"output '{name}': {msg}")
            if exp.value is not None:
                gv, rv = flat.reshape(np.asarray(exp.value).shape), np.asarray(exp.value)
                if exp.rows is not None:
                    gv, rv = gv[exp.rows], rv[exp.rows]
                msg = compare(gv, rv, exp)
                if msg:
                    problems.append(f"output '{name}': {msg}")
        missing = [a.name for a in self.arrs.values() if a.role in ("out", "inout") and a.name not in expected]
        assert not missing, f"no reference for {missing}"
        return problems


def compare(got, ref, exp):
    if got.dtype.kind in "iu" or exp.tol == "exact":
        same = got == ref.astype(got.dtype)
        if got.dtype.kind == "f":
            same = same | ((got != got) & (ref != ref))
        if not np.all(same):
            i = int(np.flatnonzero(~same.reshape(-1))[0])
            return f"{int((~same).sum())} element(s) differ from the reference (exact), first at {i}: {got.reshape(-1)[i]!r} != {ref.reshape(-1)[i]!r}"
        return None
    g, r = got.astype(np.float64), ref.astype(np.float64)
    if exp.exact_rows is not None and exp.exact_rows.any():
        rows = exp.exact_rows
        if not np.array_equal(got[rows], ref[rows].astype(got.dtype), equal_nan=True):
            return "rows the plan does not split are not bit-equal to the oracle"
    inf = ~np.isfinite(r)
    if inf.any():
        if not np.array_equal(g[inf], r[inf], equal_nan=True):
            return "non-finite entries of the reference (identities of empty rows) differ"
        g, r = np.where(inf, 0.0, g), np.where(inf, 0.0, r)
    if not np.all(np.isfinite(g)):
        return f"{int((~np.isfinite(g)).sum())} non-finite element(s) where the reference is finite"
    rtol = RTOL64 if got.dtype == np.float64 else RTOL
    floor = np.asarray(exp.scale, np.float64)
    if floor.ndim:                                   # one floor per row
        floor = floor.reshape(floor.shape + (1,) * (r.ndim - floor.ndim))
    scale = np.maximum(max(float(np.abs(r).max()) if r.size else 0.0, 1e-30), floor)
    rel = np.abs(g - r) / scale
    if r.size and float(rel.max()) > rtol:
        return f"max error {float(np.abs(g - r).max()):.3e} is {float(rel.max()):.2e} of the reference's scale (bound {rtol:g})"
    if np.linalg.norm(g - r) > rtol * max(np.linalg.norm(r), float(floor.max()) * np.sqrt(max(r.size, 1)), 1e-30):
        return f"differs from the reference norm-wise by more than {rtol:g}"
    if exp.tol == "mag":
        rel = float((np.abs(g - r) / np.maximum(exp.mag, 1e-30)).max()) if r.size else 0.0
        if rel > SPLIT_BOUND:
            return f"error {rel:.2e} of sum|w||x| exceeds SPLIT_BOUND {SPLIT_BOUND:g}"
    return None


# ------------------------------------------------------------------------------------------------------------------------------------
# graphs and plans
# ------------------------------------------------------------------------------------------------------------------------------------
class Graph:
    """COO edge index, 1-based int64 (as the reference holds it)"""

    def __init__(self, name, s, t, n_src, n_dst=None, thr=None, want_split=None):
        self.name = name
        self.s, self.t = np.asarray(s, np.int64), np.asarray(t, np.int64)
        self.n_src, self.n_dst = int(n_src), int(n_src if n_dst is None else n_dst)
        self.E = len(self.s)
        self.thr, self.want_split = thr, want_split      # hub graph: the threshold it was built for and the rows that must be split

    @property
    def n(self):
        assert self.n_src == self.n_dst
        return self.n_src

    def order(self):
        """slot order of the plan: stable sort by destination"""
        return np.argsort(self.t, kind="stable")

    def indeg(self):
        return np.bincount(self.t - 1, minlength=self.n_dst)


class Pl:
    """a plan argument: the plan of `g` (transposed: of the reversed edge index), with or without plan-added self loops"""

    def __init__(self, g, T=False, loops=False):
        self.g, self.T, self.loops = g, T, loops


class HostOut:
    def __init__(self, name, ctype=ctypes.c_int64):
        self.name, self.ctype = name, ctype


STREAM = object()


class Rec:
    """a record argument: `const gnnmp_<x>_t *job`, a HOST structure of device pointers and scalars.  fields: in the header's order, each
    an Arr (or a view of one), None (a NULL pointer), a Pl (a plan handle inside the record), a list of Rec (a nested table: the field
    points at the first of them) or a scalar"""

    def __init__(rec, ctype, /, **fields):              # positional-only: `self` is a field name of the hop's records
        rec.ctype, rec.fields = ctype, fields


class PtrTab:
    """a HOST table of device pointers (`const float *const *W_root`): a list of Arr | None, one pointer into the slab per entry, a None
    entry stays NULL.  The arrays belong to the slab like any other argument's"""

    def __init__(self, items):
        self.items = list(items)
        assert all(a is None or isinstance(a, Arr) for a in self.items)


class HostArr:
    """a plain HOST array of scalars (`const int64_t *dims`, `const int *act`): a ctypes array made at bind time"""

    def __init__(self, ctype, values):
        self.ctype, self.values = ctype, tuple(int(v) for v in values)

    def __eq__(self, other):
        return isinstance(other, HostArr) and (self.ctype, self.values) == (other.ctype, other.values)

    def __repr__(self):
        return f"HostArr({self.ctype.__name__}, {self.values})"


class Jobs:
    """a `gnnmp_chain_jobs_t *` argument.  mode 'none': NULL; 'host': gnnmp_chain_jobs_create; 'device': gnnmp_chain_jobs_pack with the
    announcement (rows, largest member, some member empty) computed here from seg_ptr, as a caller computes it from its host integers.
    The handle is built from a private device copy of seg_ptr (the call's own seg_ptr lives in the slab and may be shifted) and is
    owned by the Plans object: one handle per (mode, seg_ptr) serves every call of a test, then dies with the plans"""

    def __init__(self, mode, seg_ptr=None):
        assert mode in ("none", "host", "device") and (mode == "none" or seg_ptr is not None)
        self.mode = mode
        self.seg = None if seg_ptr is None else np.ascontiguousarray(seg_ptr, np.int64)

    def announcement(self):
        sizes = np.diff(self.seg)
        return int(self.seg[-1] - self.seg[0]), int(sizes.max()) if sizes.size else 0, int((sizes == 0).any())

    def key(self):
        return ("jobs", self.mode, None if self.seg is None else self.seg.tobytes())

    def __eq__(self, other):
        return isinstance(other, Jobs) and self.key() == other.key()

    def __repr__(self):
        return f"Jobs({self.mode!r}, G = {0 if self.seg is None else len(self.seg) - 1})"


class PlanTab:
    """a HOST table of plan handles (`const gnnmp_graph_t *const *members`): a list of Pl"""

    def __init__(self, plans):
        self.plans = list(plans)
        assert all(isinstance(p, Pl) for p in self.plans)


class NewPlan:
    """`gnnmp_graph_t **out`: a plan the CALL creates.  Its handle is a host result of the call (host[name]) and belongs to the Plans
    object from then on, which destroys it with the others"""

    def __init__(self, name="plan"):
        self.name = name


def flat_args(args):
    """the leaves of an argument list in order, records, nested tables and host tables of pointers / plans opened"""
    for a in args:
        if isinstance(a, Rec):
            yield from flat_args(a.fields.values())
        elif isinstance(a, (list, tuple)) and a and all(isinstance(r, Rec) for r in a):
            yield from flat_args(a)
        elif isinstance(a, PtrTab):
            yield from a.items
        elif isinstance(a, PlanTab):
            yield from a.plans
        else:
            yield a


def struct_of(ctype):
    """the ctypes.Structure gnnmp/_lib.py keeps for a record type (its docstring names the type)"""
    from gnnmp import _lib
    found = [c for c in vars(_lib).values() if isinstance(c, type) and issubclass(c, ctypes.Structure)
             and (c.__doc__ or "").lstrip().startswith(ctype + ":")]
    assert len(found) == 1, f"{len(found)} structures of gnnmp/_lib.py say they are {ctype}"
    return found[0]


def _struct(rec, slab, plans, keep):
    st = struct_of(rec.ctype)()
    names = [f[0] for f in st._fields_]
    assert list(rec.fields) == names, f"{rec.ctype}: the case gives {list(rec.fields)}, the structure has {names}"
    for fname, v in rec.fields.items():
        if isinstance(v, Arr):
            setattr(st, fname, slab.ptr_of(v))
        elif isinstance(v, Pl):
            setattr(st, fname, plans.get(v))
        elif isinstance(v, (list, tuple)):
            setattr(st, fname, _table(v, slab, plans, keep))
        elif v is not None:
            setattr(st, fname, v)
    keep.append(st)
    return st


def _table(recs, slab, plans, keep):
    assert recs and len({r.ctype for r in recs}) == 1
    items = [_struct(r, slab, plans, keep) for r in recs]
    tab = (type(items[0]) * len(items))(*items)          # copies: pointers only, what they point at is kept by `keep`
    keep.append(tab)
    return tab


def random_graph(name, n, E, seed, n_dst=None):
    rng = np.random.default_rng(seed)
    nd = n if n_dst is None else n_dst
    return Graph(name, rng.integers(1, n + 1, E), rng.integers(1, nd + 1, E), n, nd)


def hub_graph(thr, n=40, seed=5):
    """isolated destinations first, last and interior; one row exactly at the long-row threshold, one just above, one hub of five
    times the threshold (it spans chunks); the rest short"""
    rng = np.random.default_rng(seed)
    deg = rng.integers(1, 7, n)
    deg[[0, n // 2, n - 1]] = 0
    deg[5], deg[6], deg[7] = thr, thr + 1, 5 * thr
    t = np.repeat(np.arange(1, n + 1), deg)
    perm = rng.permutation(len(t))
    t = t[perm]
    s = rng.integers(1, n + 1, len(t))
    return Graph("hub", s, t, n, thr=int(thr), want_split=2)


class Plans:
    """plans of one test: created on first use, destroyed together (a new Plans has new plans, hence fresh workspaces)"""

    def __init__(self, lib, stream=None):
        self.lib, self.live, self.stream = lib, {}, stream
        self.live_jobs, self.created = {}, []      # jobs handles by (mode, seg_ptr); plans that calls of the test created

    def get(self, p):
        import torch
        key = (id(p.g), p.T, p.loops)
        if key in self.live:
            return self.live[key][0]
        g = p.g
        s, t, ns, nd = (g.t, g.s, g.n_dst, g.n_src) if p.T else (g.s, g.t, g.n_src, g.n_dst)
        sd, td = torch.from_numpy(s.copy()).cuda(), torch.from_numpy(t.copy()).cuda()
        h = ctypes.c_void_p()
        rc = self.lib.gnnmp_plan_create(ctypes.byref(h), ctypes.c_void_p(sd.data_ptr()), ctypes.c_void_p(td.data_ptr()), 8, 1, ns, nd, len(s),
                                        1 if p.loops else 0, 1, self.stream)
        assert rc == OK, self.lib.gnnmp_last_error()
        if g.thr is not None and not p.T and not p.loops:
            info = (ctypes.c_int64 * 8)()
            assert self.lib.gnnmp_plan_info(h, info) == OK
            assert info[7] == g.thr, f"the hub graph was built for threshold {g.thr}, the plan reports {info[7]}"
            assert info[5] == g.want_split, f"{info[5]} rows split, {g.want_split} intended"
        self.live[key] = (h, sd, td)
        return h

    def jobs(self, j):
        """the handle of a Jobs argument (None for mode 'none'): made once per (mode, seg_ptr) from a private device copy of seg_ptr"""
        import torch
        if j.mode == "none":
            return None
        key = j.key()
        if key not in self.live_jobs:
            sd = torch.from_numpy(j.seg.copy()).cuda()
            h, G = ctypes.c_void_p(), len(j.seg) - 1
            if j.mode == "host":
                rc = self.lib.gnnmp_chain_jobs_create(ctypes.byref(h), ctypes.c_void_p(sd.data_ptr()), G, self.stream)
            else:
                rc = self.lib.gnnmp_chain_jobs_pack(ctypes.byref(h), ctypes.c_void_p(sd.data_ptr()), G, *j.announcement(), self.stream)
            assert rc == OK, self.lib.gnnmp_last_error()
            torch.cuda.synchronize()               # (the device packing is asynchronous: the call under test may run on another stream)
            self.live_jobs[key] = (h, sd)
        return self.live_jobs[key][0]

    def adopt(self, h):
        """a plan handle a call of the test will create (a ctypes.c_void_p the call fills in): destroyed with the others"""
        self.created.append(h)

    def close(self):
        for h, _, _ in self.live.values():
            self.lib.gnnmp_plan_destroy(h)
        for h in self.created:
            if h.value:
                self.lib.gnnmp_plan_destroy(h)
        for h, _ in self.live_jobs.values():
            self.lib.gnnmp_chain_jobs_destroy(h)
        self.live, self.live_jobs, self.created = {}, {}, []


def plan_threshold(lib, n_edges):
    """the long-row threshold the library picks for a plan of about n_edges slots (gnnmp_plan_info's info[7])"""
    import torch
    s = torch.ones(max(n_edges, 1), dtype=torch.int64, device="cuda")
    h = ctypes.c_void_p()
    assert lib.gnnmp_plan_create(ctypes.byref(h), ctypes.c_void_p(s.data_ptr()), ctypes.c_void_p(s.data_ptr()), 8, 1, 1, 1, s.numel(), 0, 0, None) == OK
    info = (ctypes.c_int64 * 8)()
    assert lib.gnnmp_plan_info(h, info) == OK
    lib.gnnmp_plan_destroy(h)
    return int(info[7])


# ------------------------------------------------------------------------------------------------------------------------------------
# a case and its run
# ------------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, export, sid, args, ref, guard=GUARD_MIN, status=OK, align_status=None, knobs=None, no_warmup=False, then=None):
        self.export, self.sid, self.args, self.ref, self.guard, self.status = export, sid, args, ref, guard, status
        self.knobs = knobs or {}                   # gnnmp_tune settings for the call (the previous values come back after it)
        self.align_status = align_status or {}     # {array name: status the header documents for an under-aligned pointer}
        # then: (export, args) of a SECOND library call, made after the first returned OK, whose arrays belong to the same slab and whose
        # outputs the reference states too — gnnmp_plan_export of the plan the call created (args name it: Made(name))
        self.then = then
        leaves = list(flat_args(args)) + (list(flat_args(then[1])) if then else [])
        self.arrs = []                             # the arrays the slab holds: every Arr of the call, records opened; a view counts as its base
        for a in leaves:
            if isinstance(a, Arr):
                b = a if a.base is None else a.base
                if not any(b is x for x in self.arrs):
                    self.arrs.append(b)
        self.uses_plan = any(isinstance(a, Pl) for a in leaves)
        self.no_warmup = no_warmup                 # the header: "may be recorded into a HIP graph without an eager call first"


class Made:
    """in the arguments of a case's second call (Case.then): the plan the first call created through NewPlan(name)"""

    def __init__(self, name="plan"):
        self.name = name


def bind(case, slab, plans, stream=None):
    """the ctypes arguments of one call: pointers into the slab, plan handles, the stream.  Returns (arguments, host results)"""
    return bind_args(case.args, slab, plans, stream, {})


def bind_args(args, slab, plans, stream, host):
    cargs = []
    for a in args:
        if isinstance(a, PtrTab):
            tab = (ctypes.c_void_p * max(len(a.items), 1))(*[None if v is None else slab.ptr_of(v).value for v in a.items])
            cargs.append(tab)
        elif isinstance(a, HostArr):
            cargs.append((a.ctype * max(len(a.values), 1))(*a.values))
        elif isinstance(a, Jobs):
            cargs.append(plans.jobs(a))
        elif isinstance(a, PlanTab):
            cargs.append((ctypes.c_void_p * max(len(a.plans), 1))(*[plans.get(p).value for p in a.plans]))
        elif isinstance(a, NewPlan):
            h = ctypes.c_void_p()
            host[a.name] = h
            plans.adopt(h)
            cargs.append(ctypes.byref(h))
        elif isinstance(a, Made):
            cargs.append(host[a.name])
        elif isinstance(a, Arr):
            cargs.append(slab.ptr_of(a))
        elif isinstance(a, Rec) or (isinstance(a, (list, tuple)) and a and isinstance(a[0], Rec)):
            keep = []                  # the structures live as long as the argument does: byref keeps `obj`, obj keeps the rest
            if isinstance(a, Rec):
                obj = _struct(a, slab, plans, keep)
                arg = ctypes.byref(obj)                                  # (keeps obj)
            else:
                obj = _table(a, slab, plans, keep)
                arg = ctypes.cast(obj, ctypes.POINTER(obj._type_))       # a table is passed as the pointer to its first record (keeps obj)
            obj._keep = keep
            if not isinstance(a, Rec):
                arg._keep_table = obj                                    # the records of the table, for whoever inspects the call
            cargs.append(arg)
        elif isinstance(a, Pl):
            cargs.append(plans.get(a))
        elif isinstance(a, HostOut):
            v = a.ctype(-12345)
            host[a.name] = v
            cargs.append(v if isinstance(v, ctypes.Array) else ctypes.byref(v))      # (`int64_t *total` of two words: the array itself)
        elif a is STREAM:
            cargs.append(None if stream is None else ctypes.c_void_p(stream.cuda_stream))
        else:
            cargs.append(a)
    return cargs, host


def call(lib, case, cargs):
    """the one library call of a case, under its tuning knobs"""
    before = {}
    for k, v in case.knobs.items():
        was = ctypes.c_int()
        assert lib.gnnmp_tune_get(k, ctypes.byref(was), None) == OK
        before[k] = was.value
        assert lib.gnnmp_tune(k, v) == OK
    try:
        return getattr(lib, case.export)(*cargs)
    finally:
        for k, v in before.items():
            lib.gnnmp_tune(k, v)


def run_case(lib, case, plans, shifts=None, stream=None, device="cuda"):
    """one call with every array inside a fresh slab.  Returns (status, slab, host results)"""
    import torch
    slab = Slab(case.arrs, device, shifts, case.guard)
    cargs, host = bind(case, slab, plans, stream)
    if stream is not None:
        torch.cuda.synchronize()       # the default stream is idle while the side stream works
    rc = call(lib, case, cargs)
    torch.cuda.synchronize()
    if rc == OK and case.then is not None:
        export, args = case.then
        rc2 = getattr(lib, export)(*bind_args(args, slab, plans, stream, host)[0])
        torch.cuda.synchronize()
        assert rc2 == OK, f"{case.export}[{case.sid}]: {export} on the call's result returned {rc2} ({lib.gnnmp_last_error().decode()})"
    return rc, slab, {k: (v.value if hasattr(v, "value") else list(v)) for k, v in host.items()}


def verify(case, rc, slab, host):
    """problems of one finished call against the case's reference"""
    if rc != case.status:
        return [f"{case.export} returned status {rc}, expected {case.status}"]
    if rc != OK:
        return slab.check({}, untouched=True)
    return slab.check(case.ref(host))


# ------------------------------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------------------------------
import zlib

DS = (1, 2, 3, 4, 6, 7, 100, 127, 128, 129, 260)      # every vector decision and tail
IDX = ((8, 1), (4, 1), (8, 0), (4, 0))                   # (idx_bytes, index_base)
f32, f64 = np.float32, np.float64


_VARIANT = [0]      # the variant of the Ctx whose cases are being built (set by the TABLE wrappers below, read by rng_of)


class Rng:
    """the generator a case builder draws from.  Integer draws and permutations (graphs, index arrays, segment ids) always come from the
    stream seeded by the case's key alone: every variant of a case has the same graphs, shapes, index arrays and plans.  Float draws
    come from that stream for variant 0 (bit for bit the data the table always had); for any other variant they advance it all the same
    (the integer draws after them stay in step) and return values from a second stream seeded by (key, variant)"""

    def __init__(self, seed, variant):
        self.base = np.random.default_rng(seed)
        self.alt = np.random.default_rng([seed, int(variant)]) if variant else None

    def integers(self, *a, **k):
        return self.base.integers(*a, **k)

    def permutation(self, *a, **k):
        return self.base.permutation(*a, **k)

    def uniform(self, *a, **k):
        v = self.base.uniform(*a, **k)
        return v if self.alt is None else self.alt.uniform(*a, **k)

    def random(self, *a, **k):
        v = self.base.random(*a, **k)
        return v if self.alt is None else self.alt.random(*a, **k)

    def counts(self, lo, hi, n):
        """integers that are float DATA of the case (degrees), not indices: they differ between variants"""
        v = self.base.integers(lo, hi, n)
        return v if self.alt is None else self.alt.integers(lo, hi, n)


def rng_of(*key):
    return Rng(zlib.crc32(repr(key).encode()), _VARIANT[0])


def F(rng, *shape, dtype=f32):
    return rng.uniform(-1.0, 1.0, shape).astype(dtype)


def IX(idx1, ib, base):
    """a 1-based index array in the width and base of the call"""
    return (np.asarray(idx1, np.int64) - 1 + base).astype(np.int64 if ib == 8 else np.int32)


def seg_sum(idx0, vals, n):
    out = np.zeros((n,) + vals.shape[1:], f64)
    np.add.at(out, idx0, vals)
    return out


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def act64(code, x):
    if code == 0:
        return x
    if code == 1:
        return np.maximum(x, 0.0)
    if code == 2:
        return np.log1p(np.exp(-np.abs(x))) + np.maximum(x, 0.0)
    if code == 3:
        return np.tanh(x)
    return x * sigmoid(x)


class Ctx:
    """the graphs every plan-taking case runs on.  thr: the plan's long-row threshold (read from the library on the GPU; the header's
    GNNMP_MIN_LONG_ROW for the CPU dry run of the table).  variant: the same cases — graphs, shapes, index arrays, plans — with other
    float inputs, hence other references (tests/test_abi_graph_capture.py replays a captured call on them)"""

    def __init__(self, thr, variant=0):
        self.thr = int(thr)
        self.variant = int(variant)                     # salts the float inputs of every case (rng_of): 0 = the table's own data
        self.hub = hub_graph(self.thr)
        self.e0 = Graph("edgeless", [], [], 5)
        self.one = Graph("one", [1, 1], [1, 1], 1)
        self.r31 = random_graph("n31", 31, 90, 1)
        self.r33 = random_graph("n33", 33, 100, 2)
        self.r300 = random_graph("n300", 300, 900, 3)
        self.cache = {}                                 # graphs a builder makes for itself (plans are keyed on the Graph object)

    def graph_shapes(self, Ds=DS, small=(3, 128), align=(3, 6, 128), ws=(4,), rows300=(1, 260)):
        """(graph, D, tags): every width on the hub graph, two widths on the others; the 300-row graph also at the narrowest width (64 rows to
        a wave: only there does a launch have a second block of rows and a last block that is not full) and at one of several feature tiles"""
        first = True
        for D in Ds:
            tags = set()
            if D in align:
                tags.add("align")
            if D in ws:
                tags.add("ws")
            if first:
                tags.add("side")
                first = False
            yield self.hub, D, tags
        for g in (self.e0, self.one, self.r31, self.r33, self.r300):
            for D in small:
                if D in Ds:
                    yield g, D, set()
        for D in rows300:
            if D in Ds and D not in small:
                yield self.r300, D, set()

    def short_rows(self, g, loops=False):
        return (g.indeg() + (1 if loops else 0)) <= self.thr


# ---- the geometry graphs (tests/test_row_geometry.py) -----------------------------------------------------------------------------------
CHUNK_SLOTS = 128                 # csrc/plan.hip: plan_chunk_slots' default; the plan's threshold caps it
GEOM_TAILS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65)       # the tails of U = 2, 4, 8 and of G = 1 .. 64
GEOM_HUB_CHUNKS = 20              # the large hub spans more chunks than this: several fold slices at G = 32 (NG = 8), one-chunk slices at G = 1
# destinations: for rows of 21 lanes and more / for rows of one to four lanes (up to 256 to a block).  Chosen so that with 1, 2, 3 and 4
# waves a block every width of GeomCtx has at least 64 row blocks, a number of ordinary-row blocks that is no multiple of 8 and a partly
# empty last block (tests/test_row_geometry.py asserts it)
GEOM_N_WIDE, GEOM_N_NARROW = 1110, 17064


def geom_lengths(thr):
    """the row lengths a geometry graph must contain besides the three empty rows and its short random rest"""
    clen = min(int(thr), CHUNK_SLOTS)
    # each length once: at thr = 64 the tails 63, 64, 65 ARE thr - 1, thr, thr + 1.  A second row of thr + 1 would be a fourth split row,
    # and the first positions of plan->row_order past the split rows (which every row kernel skips) would never be ordinary rows
    want = GEOM_TAILS + (thr - 1, thr, thr + 1, 5 * thr + 3, GEOM_HUB_CHUNKS * clen + 1)
    return tuple(dict.fromkeys(want))


def geom_graph(name, n, thr, seed):
    """row lengths as hub_graph builds them: destinations 0, n // 2 and n - 1 empty, geom_lengths(thr) at random interior rows, the
    rest 1 .. 6; edges in random order.  Two rows hold one source only (multi-edges), and one source has more than thr edges, so the
    transposed plan has a split row too"""
    rng = np.random.default_rng(seed)
    deg = rng.integers(1, 7, n)
    want = geom_lengths(thr)
    empty = [0, n // 2, n - 1]
    free = np.setdiff1d(np.arange(n), empty)
    at = rng.permutation(free)[:len(want)]
    deg[at] = want
    deg[empty] = 0
    t = np.repeat(np.arange(1, n + 1), deg)
    t = t[rng.permutation(len(t))]
    s = rng.integers(1, n + 1, len(t))
    s[rng.permutation(len(t))[:thr + 40]] = n // 3 + 1                    # one source of more than thr edges
    for length, src in ((8, 2), (16, n - 1)):                            # multi-edges: a row whose edges all come from one source
        s[t == at[want.index(length)] + 1] = src
    g = Graph(name, s, t, n, thr=int(thr), want_split=int((deg > thr).sum()))
    g.at = dict(zip(want, at))
    return g


def n_chunks_of(lengths, thr):
    """chunk virtual rows of a plan with these row lengths (csrc/plan.hip: a row longer than thr is cut into balanced chunks of at most
    min(thr, 128) slots)"""
    clen = min(int(thr), CHUNK_SLOTS)
    lengths = np.asarray(lengths, np.int64)
    return int((-(-lengths[lengths > thr] // clen)).sum())


def lanes_of(width, C=None):
    """(vec, log2g) of a row of `width` floats at 16-byte aligned pointers (csrc/common.h: pick_vec, pick_log2g; C: the head width of
    an attention row, csrc/headgeom.h: a lane's features lie inside one head)"""
    vec = 4 if width % 4 == 0 else 2 if width % 2 == 0 else 1
    while C is not None and vec > 1 and C % vec:
        vec >>= 1
    lanes, l = -(-width // vec), 0
    while (1 << l) < lanes and l < 6:
        l += 1
    return vec, l


def walk_blocks(n_rows, n_chunks, log2g, waves):
    """(blocks, nbc, rows in the last block, rows per block) of a row walk (csrc/rowwalk.h: row_blocks, row_grid)"""
    rpb = (64 >> log2g) * waves
    total = n_rows + n_chunks
    blocks = -(-total // rpb)
    return blocks, min(blocks, -(-n_chunks // rpb)), total - (blocks - 1) * rpb, rpb


class GeomCtx:
    """Ctx for the builders of the kernels that remap, reorder and batch their row walk: the same cases on two graphs built for the
    walk's edges (geom_graph) — `narrow` for rows of one or two lanes, `wide` for rows of 25 lanes and more.  Float data comes from
    rng_of like the table's: its variant-0 stream, keyed by the graph's name, so the table's own data is untouched"""
    variant = 0

    def __init__(self, thr):
        self.thr = int(thr)
        self.wide = geom_graph("geom_wide", GEOM_N_WIDE, self.thr, 11)
        self.narrow = geom_graph("geom_narrow", GEOM_N_NARROW, self.thr, 12)
        self.cache = {}

    def widths(self):
        """(graph, row width): 1, 2 and 3 floats (one lane, vec 1 and 2), 100 (25 of 32 lanes, rows that are not whole 128-byte
        lines: no row order), 128 (row order applies), 260 (two feature tiles of 64 lanes)"""
        return [(self.narrow, 1), (self.wide, 100), (self.narrow, 3), (self.wide, 128), (self.narrow, 2), (self.wide, 260)]

    def graph_shapes(self, **_):
        for g, D in self.widths():
            yield g, D, set()

    def att_shapes(self, loops):
        """(graph, H, C, tags): 32 lanes with DPP heads, 4 lanes (16 rows to a wave), an odd head width, one lane a row"""
        yield self.wide, 8, 16, set()
        yield self.narrow, 2, 8, set()
        yield self.wide, 3, 7, set()
        yield self.narrow, 1, 1, set()

    def nn_shapes(self):
        return [(self.narrow, 3, 1, ()), (self.wide, 2, 70, ()), (self.narrow, 4, 8, ())]

    def fused_shapes(self):
        return [(self.wide, 100, 0, 100, ()), (self.wide, 128, 0, 128, ()), (self.wide, 64, 64, 128, ())]

    def short_rows(self, g, loops=False):
        return (g.indeg() + (1 if loops else 0)) <= self.thr


def row_shapes(Ds=DS, small=(3, 128), align=(3, 6, 128)):
    first = True
    for D in Ds:
        tags = {"align"} if D in align else set()
        if first:
            tags.add("side")
            first = False
        yield 33, D, tags
    for N in (1, 31, 300):
        for D in small:
            if D in Ds:
                yield N, D, set()


def mk(export, sid, tags, args, ref, **kw):
    c = Case(export, sid, args, ref, **kw)
    c.tags = set(tags)
    return c


def orc():
    from oracle import oracle as o
    o.build()
    return o


TABLE = {}


def cases_of(export):
    def deco(fn):
        TABLE[export] = fn
        return fn
    return deco


# ---- leaves ----------------------------------------------------------------------------------------------------------------------
def _gather(export, dt):
    def build(ctx):
        k = 0
        for K, D, tags in row_shapes():
            for ib, base in (IDX if D == 3 and K == 33 else (IDX[k % 4],)):
                k += 1
                r = rng_of(export, K, D, ib, base)
                n = 50
                x = F(r, n, D, dtype=dt)
                idx1 = r.integers(1, n + 1, K)
                ref = lambda host, x=x, idx1=idx1: {"out": E(orc().gather(x, idx1), "exact")}
                yield mk(export, f"K{K}_D{D}_i{ib}b{base}", tags if (ib, base) == IDX[(k - 1) % 4] else (),
                         [Arr("x", "in", x), Arr("idx", "in", IX(idx1, ib, base)), ib, base, K, Arr("out", "out", shape=(K, D), dtype=dt), D, STREAM], ref)
    return build


TABLE["gnnmp_gather_f32"] = _gather("gnnmp_gather_f32", f32)
TABLE["gnnmp_gather_f64"] = _gather("gnnmp_gather_f64", f64)


@cases_of("gnnmp_edge_sub_f32")
def _(ctx):
    for k, (K, D, tags) in enumerate(row_shapes()):
        ib, base = IDX[k % 4]
        r = rng_of("edge_sub", K, D)
        n = 40
        xi, xj = F(r, n, D), F(r, n, D)
        s1, t1 = r.integers(1, n + 1, K), r.integers(1, n + 1, K)
        flag = k % 2
        d = xi.astype(f64)[t1 - 1] - xj.astype(f64)[s1 - 1]
        ref = lambda host, d=d, flag=flag: {"out": -d if flag else d}
        yield mk("gnnmp_edge_sub_f32", f"K{K}_D{D}_f{flag}", tags,
                 [Arr("xi", "in", xi), Arr("xj", "in", xj), Arr("s", "in", IX(s1, ib, base)), Arr("t", "in", IX(t1, ib, base)), ib, base, K, flag,
                  Arr("out", "out", shape=(K, D)), D, STREAM], ref)


def _scatter(export, dt):
    def build(ctx):
        for k, (g, D, tags) in enumerate(ctx.graph_shapes()):
            aggr = k % 4
            r = rng_of(export, g.name, D)
            m = F(r, g.E, D, dtype=dt)
            def ref(host, g=g, m=m, aggr=aggr):
                v = orc().scatter(aggr, m, g.t, g.n_dst)
                return {"out": E(v, "rel" if aggr in (SUM, MEAN) else "exact", exact_rows=ctx.short_rows(g))}
            yield mk(export, f"{g.name}_D{D}_a{aggr}", tags, [Pl(g), aggr, Arr("m", "in", m), Arr("out", "out", shape=(g.n_dst, D), dtype=dt), D, STREAM], ref)
    return build


TABLE["gnnmp_scatter_f32"] = _scatter("gnnmp_scatter_f32", f32)
TABLE["gnnmp_scatter_f64"] = _scatter("gnnmp_scatter_f64", f64)


@cases_of("gnnmp_scatter_atomic_f32")
def _(ctx):
    for k, (K, D, tags) in enumerate(row_shapes()):
        ib, base = IDX[k % 4]
        aggr = (SUM, MAX, MIN)[k % 3]
        r = rng_of("scatter_atomic", K, D)
        n = 7
        m = F(r, K, D)
        idx1 = r.integers(1, n + 1, K)
        init = np.full((n, D), {SUM: 0.0, MAX: -np.inf, MIN: np.inf}[aggr], f32)
        def ref(host, m=m, idx1=idx1, aggr=aggr, init=init, n=n):
            out = init.astype(f64)
            fn = {SUM: np.add, MAX: np.maximum, MIN: np.minimum}[aggr]
            fn.at(out, idx1 - 1, m.astype(f64))
            return {"out": out}
        yield mk("gnnmp_scatter_atomic_f32", f"K{K}_D{D}_a{aggr}", tags,
                 [aggr, Arr("m", "in", m), Arr("idx", "in", IX(idx1, ib, base)), ib, base, K, Arr("out", "inout", init), D, STREAM], ref)


@cases_of("gnnmp_edge_dot_f32")
def _(ctx):
    for k, (K, D, tags) in enumerate(row_shapes()):
        ib, base = IDX[k % 4]
        r = rng_of("edge_dot", K, D)
        n = 40
        a, b = F(r, n, D), F(r, n, D)
        s1, t1 = r.integers(1, n + 1, K), r.integers(1, n + 1, K)
        v = (a.astype(f64)[t1 - 1] * b.astype(f64)[s1 - 1]).sum(1)
        yield mk("gnnmp_edge_dot_f32", f"K{K}_D{D}", tags,
                 [Arr("a_dst", "in", a), Arr("b_src", "in", b), Arr("src", "in", IX(s1, ib, base)), Arr("dst", "in", IX(t1, ib, base)), ib, base, K, D,
                  Arr("out", "out", shape=(K,)), STREAM], lambda host, v=v: {"out": v})


@cases_of("gnnmp_edge_dot_plan_f32")
def _(ctx):
    for g, D, tags in ctx.graph_shapes():
        r = rng_of("edge_dot_plan", g.name, D)
        a, b = F(r, g.n_dst, D), F(r, g.n_src, D)
        v = (a.astype(f64)[g.t - 1] * b.astype(f64)[g.s - 1]).sum(1)
        yield mk("gnnmp_edge_dot_plan_f32", f"{g.name}_D{D}", tags,
                 [Pl(g), Arr("a_dst", "in", a), Arr("b_src", "in", b), Arr("out", "out", shape=(g.E,)), D, STREAM], lambda host, v=v: {"out": v},
                 # the header: the row must fit one wave at the widest lane D and the two pointers admit, else GNNMP_EUNSUPPORTED
                 status=EUNSUPPORTED if g.E and -(-D // (4 if D % 4 == 0 else 2 if D % 2 == 0 else 1)) > 64 else OK,
                 align_status={"a_dst": EUNSUPPORTED, "b_src": EUNSUPPORTED})


@cases_of("gnnmp_edge_dot_grad_f32")
def _(ctx):
    for g, D, tags in ctx.graph_shapes():
        r = rng_of("edge_dot_grad", g.name, D)
        xi, xj, dz = F(r, g.n, D), F(r, g.n, D), F(r, g.E)
        def ref(host, g=g, xi=xi, xj=xj, dz=dz):
            z = dz.astype(f64)[:, None]
            return {"dxi": seg_sum(g.t - 1, z * xj.astype(f64)[g.s - 1], g.n), "dxj": seg_sum(g.s - 1, z * xi.astype(f64)[g.t - 1], g.n)}
        yield mk("gnnmp_edge_dot_grad_f32", f"{g.name}_D{D}", tags,
                 [Pl(g), Pl(g, T=True), Arr("xi", "in", xi), Arr("xj", "in", xj), Arr("dz", "in", dz), Arr("dxi", "out", shape=(g.n, D)),
                  Arr("dxj", "out", shape=(g.n, D)), D, STREAM], ref, status=EUNSUPPORTED if D > 256 else OK)


# ---- propagate -------------------------------------------------------------------------------------------------------------------
def _prop_ref(ctx, g, aggr, x, w, ss, sd):
    """the reference's materialised sequence xj .* cout' -> propagate -> x .* cin' (float32 oracle, bit-exact on unsplit rows)"""
    o = orc()
    xs = o.scale_rows(x, ss) if ss is not None and x.dtype == f32 else (x if ss is None else x * ss[:, None])
    y = o.propagate(aggr, g.s, g.t, g.n_src, xs, w, n_dst=g.n_dst)
    if sd is not None:
        y = o.scale_rows(y, sd) if y.dtype == f32 else y * sd[:, None]
    # max / min: every bit on every row, split rows included (tests/test_gpu_parity.py, tests/test_float64.py); + / mean: every bit on the
    # rows the plan does not split, the parity bound on the split ones
    return E(y, "exact" if aggr in (MAX, MIN) else "rel", exact_rows=ctx.short_rows(g))


def _propagate(export, dt):
    def build(ctx):
        for k, (g, D, tags) in enumerate(ctx.graph_shapes()):
            msg, aggr, scaled = ((0, SUM, False), (1, SUM, True), (0, MAX, False), (0, MEAN, False), (1, MIN, False), (0, SUM, True))[k % 6]
            r = rng_of(export, g.name, D)
            x = F(r, g.n_src, D, dtype=dt)
            w = F(r, g.E, dtype=dt) if msg else None
            ss = (0.5 + r.random(g.n_src)).astype(dt) if scaled else None
            sd = (0.5 + r.random(g.n_dst)).astype(dt) if scaled else None
            ref = lambda host, g=g, aggr=aggr, x=x, w=w, ss=ss, sd=sd: {"out": _prop_ref(ctx, g, aggr, x, w, ss, sd)}
            yield mk(export, f"{g.name}_D{D}_m{msg}a{aggr}s{int(scaled)}", tags,
                     [Pl(g), msg, aggr, Arr("xj", "in", x), Arr("w", "in", w) if msg else None, Arr("scale_src", "in", ss) if scaled else None,
                      Arr("scale_dst", "in", sd) if scaled else None, Arr("out", "out", shape=(g.n_dst, D), dtype=dt), D, STREAM], ref)
    return build


TABLE["gnnmp_propagate_f32"] = _propagate("gnnmp_propagate_f32", f32)
TABLE["gnnmp_propagate_f64"] = _propagate("gnnmp_propagate_f64", f64)


def _slots(export, with_act):
    def build(ctx):
        for k, (g, D, tags) in enumerate(ctx.graph_shapes()):
            aggr = (SUM, MEAN, MAX)[k % 3]
            scaled = aggr == SUM
            r = rng_of(export, g.name, D)
            x, w = F(r, g.n_src, D), F(r, g.E)
            ss = (0.5 + r.random(g.n_src)).astype(f32) if scaled else None
            sd = (0.5 + r.random(g.n_dst)).astype(f32) if scaled else None
            order = g.order()
            w_slot = w[order]
            ss_slot = ss[g.s[order] - 1] if scaled else None
            bias = F(r, D) if with_act and k % 2 == 0 else None
            act = k % 2 if with_act else 0
            def ref(host, g=g, aggr=aggr, x=x, w=w, ss=ss, sd=sd, bias=bias, act=act):
                e = _prop_ref(ctx, g, aggr, x, w, ss, sd)
                if with_act:
                    v = e.value if bias is None else (e.value + bias[None, :]).astype(f32)
                    e.value = np.maximum(v, 0) if act else v
                return {"out": e}
            args = [Pl(g), aggr, Arr("xj", "in", x), Arr("w_slot", "in", w_slot), Arr("ss_slot", "in", ss_slot) if scaled else None,
                    Arr("scale_dst", "in", sd) if scaled else None]
            if with_act:
                args += [Arr("bias", "in", bias) if bias is not None else None, act]
            yield mk(export, f"{g.name}_D{D}_a{aggr}", tags, args + [Arr("out", "out", shape=(g.n_dst, D)), D, STREAM], ref)
    return build


TABLE["gnnmp_propagate_slots_f32"] = _slots("gnnmp_propagate_slots_f32", False)
TABLE["gnnmp_propagate_slots_act_f32"] = _slots("gnnmp_propagate_slots_act_f32", True)


@cases_of("gnnmp_plan_slot_gather_f32")
def _(ctx):
    for k, g in enumerate((ctx.hub, ctx.e0, ctx.one, ctx.r31, ctx.r33, ctx.r300)):
        for by in (0, 1):
            r = rng_of("slot_gather", g.name, by)
            v = F(r, g.E if by else g.n_src)
            order = g.order()
            val = v[order] if by else v[g.s[order] - 1]
            yield mk("gnnmp_plan_slot_gather_f32", f"{g.name}_by{by}", {"align", "ws"} | ({"side"} if k == 0 and by == 0 else set()) if g is ctx.hub else (),
                     [Pl(g), by, Arr("v", "in", v), Arr("out_slot", "out", shape=(g.E,)), STREAM], lambda host, val=val: {"out_slot": E(val, "exact")})


@cases_of("gnnmp_propagate_emul_f32")
def _(ctx):
    for k, (g, D, tags) in enumerate(ctx.graph_shapes()):
        aggr = (SUM, MEAN, MAX, MIN)[k % 4]
        r = rng_of("emul", g.name, D)
        x, e = F(r, g.n_src, D), F(r, g.E, D)
        ref = lambda host, g=g, aggr=aggr, x=x, e=e: {"out": orc().scatter(aggr, e.astype(f64) * x.astype(f64)[g.s - 1], g.t, g.n_dst)}
        yield mk("gnnmp_propagate_emul_f32", f"{g.name}_D{D}_a{aggr}", tags,
                 [Pl(g), aggr, Arr("xj", "in", x), Arr("e", "in", e), Arr("out", "out", shape=(g.n_dst, D)), D, STREAM], ref)


@cases_of("gnnmp_propagate_gated_f32")
def _(ctx):
    for k, (g, D, tags) in enumerate(ctx.graph_shapes()):
        aggr = (SUM, MEAN, MAX)[k % 3]
        r = rng_of("gated", g.name, D)
        gi, bv = F(r, g.n_dst, D), F(r, g.n_src, 2 * D)
        def ref(host, g=g, aggr=aggr, gi=gi, bv=bv, D=D):
            b = bv.astype(f64)[g.s - 1]
            return {"out": orc().scatter(aggr, sigmoid(gi.astype(f64)[g.t - 1] + b[:, :D]) * b[:, D:], g.t, g.n_dst)}
        yield mk("gnnmp_propagate_gated_f32", f"{g.name}_D{D}_a{aggr}", tags,
                 [Pl(g), aggr, Arr("gate_i", "in", gi), Arr("bv_j", "in", bv), Arr("out", "out", shape=(g.n_dst, D)), D, STREAM], ref)


@cases_of("gnnmp_propagate_cg_f32")
def _(ctx):
    for k, (g, D, tags) in enumerate(ctx.graph_shapes()):
        act = (2, 0, 1, 3)[k % 4]
        has_e = k % 2 == 0
        r = rng_of("cg", g.name, D)
        fi, fj = F(r, g.n_dst, 2 * D), F(r, g.n_src, 2 * D)
        fe = F(r, g.E, 2 * D) if has_e else None
        def ref(host, g=g, fi=fi, fj=fj, fe=fe, act=act, D=D):
            z = fi.astype(f64)[g.t - 1] + fj.astype(f64)[g.s - 1] + (fe.astype(f64) if fe is not None else 0.0)
            return {"out": seg_sum(g.t - 1, sigmoid(z[:, :D]) * act64(act, z[:, D:]), g.n_dst)}
        yield mk("gnnmp_propagate_cg_f32", f"{g.name}_D{D}_act{act}", tags,
                 [Pl(g), Arr("fs_i", "in", fi), Arr("fs_j", "in", fj), Arr("fs_e", "in", fe) if has_e else None, act,
                  Arr("out", "out", shape=(g.n_dst, D)), D, STREAM], ref)


@cases_of("gnnmp_propagate_nn_f32")
def _(ctx):
    shapes = ctx.nn_shapes() if hasattr(ctx, "nn_shapes") else \
             [(ctx.hub, 3, 5, {"align", "side", "ws"}), (ctx.hub, 4, 4, {"align"}), (ctx.hub, 7, 2, ()), (ctx.hub, 1, 1, ()), (ctx.hub, 6, 33, {"align"}),
              (ctx.e0, 3, 4, ()), (ctx.one, 4, 3, ()), (ctx.r31, 2, 6, ()), (ctx.r33, 5, 3, ()), (ctx.r300, 4, 8, ()),
              (ctx.r300, 3, 1, ()), (ctx.r300, 2, 70, ())]         # 64 rows to a wave; two feature tiles (a lane per output feature)
    for k, (g, Din, Dout, tags) in enumerate(shapes):
        aggr = (SUM, MEAN, MAX)[k % 3]
        r = rng_of("nn", g.name, Din, Dout)
        x, we = F(r, g.n_src, Din), F(r, g.E, Dout * Din)
        def ref(host, g=g, x=x, we=we, Din=Din, Dout=Dout, aggr=aggr):
            W = we.astype(f64).reshape(g.E, Din, Dout)               # element (o, c) of edge k at we[k][o + Dout * c]
            msg = np.einsum("kco,kc->ko", W, x.astype(f64)[g.s - 1])
            return {"out": orc().scatter(aggr, msg, g.t, g.n_dst)}
        yield mk("gnnmp_propagate_nn_f32", f"{g.name}_{Din}x{Dout}_a{aggr}", tags,
                 [Pl(g), aggr, Arr("xj", "in", x), Arr("we", "in", we), Arr("out", "out", shape=(g.n_dst, Dout)), Din, Dout, STREAM], ref)


@cases_of("gnnmp_propagate_add_mask_f32")
def _(ctx):
    for k, (g, D, tags) in enumerate(ctx.graph_shapes()):
        aggr = (SUM, MEAN)[k % 2]
        r = rng_of("add_mask", g.name, D)
        x, add, my = F(r, g.n_src, D), F(r, g.n_dst, D), F(r, g.n_dst, D)
        sd = (1.0 / np.maximum(g.indeg(), 1)).astype(f32) if aggr == MEAN else None
        has_add, has_mask = k % 3 != 1, k % 3 != 2
        def ref(host, g=g, x=x, add=add, my=my, sd=sd, has_add=has_add, has_mask=has_mask):
            y = seg_sum(g.t - 1, x.astype(f64)[g.s - 1], g.n_dst)
            if sd is not None:
                y = y * sd.astype(f64)[:, None]
            if has_add:
                y = y + add.astype(f64)
            return {"out": np.where(my > 0, y, 0.0) if has_mask else y}
        # MEAN is `+` with scale_dst = 1 / count, as the header describes it
        yield mk("gnnmp_propagate_add_mask_f32", f"{g.name}_D{D}_a{aggr}", tags,
                 [Pl(g), SUM, Arr("xj", "in", x), Arr("scale_dst", "in", sd) if sd is not None else None, Arr("addend", "in", add) if has_add else None,
                  Arr("mask_y", "in", my) if has_mask else None, Arr("out", "out", shape=(g.n_dst, D)), D, STREAM], ref)


@cases_of("gnnmp_propagate_maxmin_grad_f32")
def _(ctx):
    for k, (g, D, tags) in enumerate(ctx.graph_shapes()):
        aggr = (MAX, MIN)[k % 2]
        r = rng_of("maxmin_grad", g.name, D)
        x, dy = np.round(F(r, g.n, D) * 4) / 4, F(r, g.n, D)          # quarter steps: ties happen, and all of them receive Δ
        x = x.astype(f32)
        y = orc().propagate(aggr, g.s, g.t, g.n, x)
        def ref(host, g=g, x=x, y=y, dy=dy):
            hit = x[g.s - 1] == y[g.t - 1]
            return {"dx": seg_sum(g.s - 1, np.where(hit, dy.astype(f64)[g.t - 1], 0.0), g.n)}
        yield mk("gnnmp_propagate_maxmin_grad_f32", f"{g.name}_D{D}_a{aggr}", tags,
                 [Pl(g, T=True), Arr("x", "in", x), Arr("y", "in", y), Arr("dy", "in", dy), Arr("dx", "out", shape=(g.n, D)), D, STREAM], ref)


@cases_of("gnnmp_degree_f32")
def _(ctx):
    for k, g in enumerate((ctx.hub, ctx.e0, ctx.one, ctx.r31, ctx.r33, ctx.r300)):
        for weighted in (0, 1):
            w = F(rng_of("degree", g.name), g.E) if weighted else None
            def ref(host, g=g, w=w):
                return {"deg": E(orc().degree(g.t, g.n_dst, w), "exact" if w is None else "rel", exact_rows=None if w is None else ctx.short_rows(g))}
            yield mk("gnnmp_degree_f32", f"{g.name}_w{weighted}", ({"align", "ws"} | ({"side"} if not weighted else set())) if g is ctx.hub else (),
                     [Pl(g), Arr("w", "in", w) if weighted else None, Arr("deg", "out", shape=(g.n_dst,)), STREAM], ref)


# ---- pointwise -------------------------------------------------------------------------------------------------------------------
NS = ((1, ()), (3, {"align"}), (6, {"align"}), (31, ()), (33, ()), (128, {"align", "side"}), (1025, ()), (70001, ()))


@cases_of("gnnmp_inv_sqrt_f32")
def _(ctx):
    for n, tags in NS:
        d = (1.0 + rng_of("inv_sqrt", n).counts(0, 50, n)).astype(f32)
        yield mk("gnnmp_inv_sqrt_f32", f"n{n}", tags, [Arr("deg", "in", d), Arr("out", "out", shape=(n,)), n, STREAM],
                 lambda host, d=d: {"out": E(orc().inv_sqrt(d), "exact")})


@cases_of("gnnmp_add_f32")
def _(ctx):
    for n, tags in NS:
        r = rng_of("add", n)
        a, b = F(r, n), F(r, n)
        yield mk("gnnmp_add_f32", f"n{n}", tags, [Arr("a", "in", a), Arr("b", "in", b), Arr("out", "out", shape=(n,)), n, STREAM],
                 lambda host, a=a, b=b: {"out": a.astype(f64) + b})


@cases_of("gnnmp_axpy_f32")
def _(ctx):
    for n, tags in NS:
        r = rng_of("axpy", n)
        x, y = F(r, n), F(r, n)
        yield mk("gnnmp_axpy_f32", f"n{n}", tags, [1.25, Arr("x", "in", x), Arr("y", "in", y), Arr("out", "out", shape=(n,)), n, STREAM],
                 lambda host, x=x, y=y: {"out": 1.25 * x.astype(f64) + y})


@cases_of("gnnmp_act_grad_f32")
def _(ctx):
    for k, (n, tags) in enumerate(NS):
        r = rng_of("act_grad", n)
        dy, y = F(r, n), F(r, n)
        act = k % 2
        yield mk("gnnmp_act_grad_f32", f"n{n}_act{act}", tags, [Arr("dy", "in", dy), Arr("y", "in", y), act, Arr("dz", "out", shape=(n,)), n, STREAM],
                 lambda host, dy=dy, y=y, act=act: {"dz": E(np.where(y > 0, dy, 0).astype(f32) if act else dy, "exact")})


@cases_of("gnnmp_mul_rows_f32")
def _(ctx):
    for k, (N, D, tags) in enumerate(row_shapes()):
        Da = 1 if k % 2 == 0 else D
        r = rng_of("mul_rows", N, D)
        a, b = F(r, N, Da), F(r, N, D)
        yield mk("gnnmp_mul_rows_f32", f"N{N}_D{D}_Da{Da}", tags, [Arr("a", "in", a), Da, Arr("b", "in", b), Arr("out", "out", shape=(N, D)), N, D, STREAM],
                 lambda host, a=a, b=b: {"out": a.astype(f64) * b})


@cases_of("gnnmp_bias_act_f32")
def _(ctx):
    for k, (N, D, tags) in enumerate(row_shapes()):
        act = k % 5
        r = rng_of("bias_act", N, D)
        x = F(r, N, D)
        bias = F(r, D) if k % 3 else None
        yield mk("gnnmp_bias_act_f32", f"N{N}_D{D}_act{act}", tags,
                 [Arr("x", "in", x), Arr("bias", "in", bias) if bias is not None else None, act, Arr("out", "out", shape=(N, D)), N, D, STREAM],
                 lambda host, x=x, bias=bias, act=act: {"out": act64(act, x.astype(f64) + (0.0 if bias is None else bias.astype(f64)))})


@cases_of("gnnmp_rowdot_f32")
def _(ctx):
    for N, D, tags in row_shapes():
        r = rng_of("rowdot", N, D)
        a, b = F(r, N, D), F(r, N, D)
        yield mk("gnnmp_rowdot_f32", f"N{N}_D{D}", tags, [Arr("a", "in", a), Arr("b", "in", b), Arr("out", "out", shape=(N,)), N, D, STREAM],
                 lambda host, a=a, b=b: {"out": (a.astype(f64) * b).sum(1)})


@cases_of("gnnmp_row_normalize_f32")
def _(ctx):
    for k, (N, D, tags) in enumerate(row_shapes()):
        x = F(rng_of("row_normalize", N, D), N, D) + f32(0.05)
        keep = k % 2 == 0
        def ref(host, x=x, keep=keep):
            nrm = np.sqrt((x.astype(f64) ** 2).sum(1))
            out = {"xn": x / nrm[:, None]}
            if keep:
                out["rnorm"] = nrm
            return out
        yield mk("gnnmp_row_normalize_f32", f"N{N}_D{D}_r{int(keep)}", tags,
                 [Arr("x", "in", x), Arr("xn", "out", shape=(N, D)), Arr("rnorm", "out", shape=(N,)) if keep else None, N, D, STREAM], ref)


@cases_of("gnnmp_row_normalize_grad_f32")
def _(ctx):
    for k, (N, D, tags) in enumerate(row_shapes()):
        r = rng_of("row_normalize_grad", N, D)
        x = F(r, N, D) + f32(0.05)
        nrm = np.sqrt((x.astype(f64) ** 2).sum(1))
        xn, rn = (x / nrm[:, None]).astype(f32), nrm.astype(f32)
        dq, dk, base = F(r, N, D), F(r, N, D), F(r, N, D)
        has_k, has_b, has_q = k % 2 == 0, k % 3 == 0, k % 2 == 1
        def ref(host, xn=xn, rn=rn, dq=dq, dk=dk, base=base, has_k=has_k, has_b=has_b, has_q=has_q):
            dn = dq.astype(f64) + (dk if has_k else 0.0)
            x64 = xn.astype(f64)
            dx = (dn - x64 * (x64 * dn).sum(1, keepdims=True)) / rn.astype(f64)[:, None] + (base if has_b else 0.0)
            out = {"dx": dx}
            if has_q:
                out["qdot"] = 0.5 * (x64 * dq).sum(1)
            return out
        yield mk("gnnmp_row_normalize_grad_f32", f"N{N}_D{D}_{int(has_k)}{int(has_b)}{int(has_q)}", tags,
                 [Arr("dq", "in", dq), Arr("dk", "in", dk) if has_k else None, Arr("xn", "in", xn), Arr("rnorm", "in", rn),
                  Arr("base", "in", base) if has_b else None, Arr("dx", "out", shape=(N, D)), Arr("qdot", "out", shape=(N,)) if has_q else None, 0.5, N, D, STREAM], ref)


@cases_of("gnnmp_row_sqnorm_normalize_f32")
def _(ctx):
    for N, D, tags in row_shapes():
        x = F(rng_of("row_sqnorm", N, D), N, D)
        def ref(host, x=x):
            sq = (x.astype(f64) ** 2).sum(1)
            return {"sq": sq, "xn": x / (np.sqrt(sq) + 1e-6)[:, None]}
        yield mk("gnnmp_row_sqnorm_normalize_f32", f"N{N}_D{D}", tags,
                 [Arr("x", "in", x), Arr("sq", "out", shape=(N,)), Arr("xn", "out", shape=(N, D)), 1e-6, N, D, STREAM], ref)


HC = ((3, 7, {"align", "side"}), (3, 6, {"align"}), (5, 4, {"align"}), (1, 1, ()), (2, 33, ()), (8, 8, ()))     # (H, C): C odd, C % 4 == 2, C % 4 == 0; H not a power of two


@cases_of("gnnmp_head_mean_f32")
def _(ctx):
    for k, (H, C, tags) in enumerate(HC):
        for N in ((33,) if k else (1, 31, 33, 300)):
            r = rng_of("head_mean", H, C, N)
            y, bias = F(r, N, H, C), F(r, C)
            act = k % 2
            yield mk("gnnmp_head_mean_f32", f"N{N}_H{H}_C{C}", tags if N == 33 else (),
                     [Arr("y", "in", y), Arr("bias", "in", bias), act, Arr("out", "out", shape=(N, C)), N, H, C, STREAM],
                     lambda host, y=y, bias=bias, act=act: {"out": act64(act, y.astype(f64).mean(1) + bias)})


@cases_of("gnnmp_head_mean_grad_f32")
def _(ctx):
    for k, (H, C, tags) in enumerate(HC):
        for N in ((33,) if k else (1, 31, 33, 300)):
            dz = F(rng_of("head_mean_grad", H, C, N), N, C)
            yield mk("gnnmp_head_mean_grad_f32", f"N{N}_H{H}_C{C}", tags if N == 33 else (),
                     [Arr("dz", "in", dz), Arr("dy", "out", shape=(N, H, C)), N, H, C, STREAM],
                     lambda host, dz=dz, H=H: {"dy": np.repeat(dz.astype(f64)[:, None, :] / H, H, 1)})


@cases_of("gnnmp_gmm_weights_f32")
def _(ctx):
    for k, (E_, ein, K, C, tags) in enumerate(((33, 3, 2, 5, {"align", "side"}), (1, 1, 1, 1, ()), (31, 2, 3, 4, {"align"}), (300, 4, 3, 6, {"align"}), (33, 5, 1, 7, ()))):
        r = rng_of("gmm", E_, ein, K, C)
        e, mu, si = F(r, E_, ein), F(r, K, ein), F(r, K, ein)
        def ref(host, e=e, mu=mu, si=si, C=C):
            # exp(+Σ ...) exactly as the reference writes it (conv.jl:379-385; oracle/more_layers.py gmm_conv)
            w = np.exp((((e.astype(f64)[:, None, :] - mu.astype(f64)[None]) ** 2 / 2) * si.astype(f64)[None] ** 2).sum(-1))
            return {"out": np.repeat(w[:, :, None], C, 2).reshape(len(e), -1)}
        yield mk("gnnmp_gmm_weights_f32", f"E{E_}_{ein}_{K}_{C}", tags,
                 [Arr("e", "in", e), Arr("mu", "in", mu), Arr("sigma_inv", "in", si), Arr("out", "out", shape=(E_, K * C)), E_, ein, K, C, STREAM], ref)


@cases_of("gnnmp_gru_pointwise_f32")
def _(ctx):
    for k, (N, D, tags) in enumerate(row_shapes()):
        r = rng_of("gru", N, D)
        gx, gh, h = F(r, N, 3 * D), F(r, N, 3 * D), F(r, N, D)
        b = F(r, 3 * D) if k % 2 == 0 else None
        def ref(host, gx=gx, gh=gh, h=h, b=b, D=D):
            bb = np.zeros(3 * D) if b is None else b.astype(f64)
            X, Hh = gx.astype(f64) + bb, gh.astype(f64)
            rr = sigmoid(X[:, :D] + Hh[:, :D])
            z = sigmoid(X[:, D:2 * D] + Hh[:, D:2 * D])
            ht = np.tanh(X[:, 2 * D:] + rr * Hh[:, 2 * D:])
            return {"out": (1 - z) * ht + z * h}
        yield mk("gnnmp_gru_pointwise_f32", f"N{N}_D{D}", tags,
                 [Arr("gx", "in", gx), Arr("gh", "in", gh), Arr("b", "in", b) if b is not None else None, Arr("h", "in", h), Arr("out", "out", shape=(N, D)), N, D, STREAM], ref)


@cases_of("gnnmp_lstm_pointwise_f32")
def _(ctx):
    for k, (N, D, tags) in enumerate(row_shapes()):
        r = rng_of("lstm", N, D)
        gx, gh, c = F(r, N, 4 * D), F(r, N, 4 * D), F(r, N, D)
        b = F(r, 4 * D) if k % 2 == 0 else None
        def ref(host, gx=gx, gh=gh, c=c, b=b, D=D):
            g = gx.astype(f64) + gh + (0.0 if b is None else b.astype(f64))
            i, f, cc, o = (g[:, j * D:(j + 1) * D] for j in range(4))
            cn = sigmoid(f) * c + sigmoid(i) * np.tanh(cc)
            return {"c_out": cn, "h_out": sigmoid(o) * np.tanh(cn)}
        yield mk("gnnmp_lstm_pointwise_f32", f"N{N}_D{D}", tags,
                 [Arr("gx", "in", gx), Arr("gh", "in", gh), Arr("b", "in", b) if b is not None else None, Arr("c", "in", c),
                  Arr("h_out", "out", shape=(N, D)), Arr("c_out", "out", shape=(N, D)), N, D, STREAM], ref)


# ---- pooling ---------------------------------------------------------------------------------------------------------------------
def _segments(r, N, G):
    """a sorted 1-based indicator with an empty first / interior / last segment when G allows"""
    ids = np.sort(r.integers(2 if G > 3 else 1, (G - 1 if G > 3 else G) + 1, N))
    if G > 4:
        ids[ids == G // 2] = G // 2 + 1
    return np.sort(ids)


def _pool(export, ptr_form):
    def build(ctx):
        for k, (N, D, tags) in enumerate(row_shapes()):
            aggr = k % 4
            ib, base = IDX[k % 4]
            G = 1 if N == 1 else 9
            r = rng_of(export, N, D)
            x = F(r, N, D)
            ids = _segments(r, N, G)
            ref = lambda host, aggr=aggr, ids=ids, x=x, G=G: {"out": E(orc().scatter(aggr, x, ids, G), "rel" if aggr < 2 else "exact")}
            if ptr_form:
                seg_ptr = np.searchsorted(ids, np.arange(1, G + 2)).astype(np.int64)
                args = [aggr, Arr("x", "in", x), Arr("seg_ptr", "in", seg_ptr), Arr("out", "out", shape=(G, D)), D, N, G, STREAM]
            else:
                args = [aggr, Arr("x", "in", x), Arr("seg_ids", "in", IX(ids, ib, base)), ib, base, Arr("out", "out", shape=(G, D)), D, N, G, STREAM]
            yield mk(export, f"N{N}_D{D}_a{aggr}", tags, args, ref)
    return build


TABLE["gnnmp_segment_pool_f32"] = _pool("gnnmp_segment_pool_f32", False)
TABLE["gnnmp_segment_pool_ptr_f32"] = _pool("gnnmp_segment_pool_ptr_f32", True)


@cases_of("gnnmp_segment_bounds")
def _(ctx):
    for k, N in enumerate((1, 31, 33, 300, 5000)):
        ib, base = IDX[k % 4]
        G = 1 if N == 1 else 9
        ids = _segments(rng_of("bounds", N), N, G)
        v = np.searchsorted(ids, np.arange(1, G + 2)).astype(np.int64)
        yield mk("gnnmp_segment_bounds", f"N{N}", {"align"} | ({"side"} if k == 2 else set()),
                 [Arr("seg_ids", "in", IX(ids, ib, base)), ib, base, N, G, Arr("seg_ptr", "out", shape=(G + 1,), dtype=np.int64), STREAM],
                 lambda host, v=v: {"seg_ptr": E(v, "exact")})


@cases_of("gnnmp_pool_grad_act_f32")
def _(ctx):
    for k, (N, D, tags) in enumerate(row_shapes()):
        ib, base = IDX[k % 4]
        act, has_inv = k % 2, k % 3 == 0
        G = 1 if N == 1 else 9
        r = rng_of("pool_grad", N, D)
        ids = _segments(r, N, G)
        dpool, y, inv = F(r, G, D), F(r, N, D), (0.1 + r.random(G)).astype(f32)
        def ref(host, ids=ids, dpool=dpool, y=y, inv=inv, act=act, has_inv=has_inv):
            v = dpool.astype(f64)[ids - 1] * (inv.astype(f64)[ids - 1][:, None] if has_inv else 1.0)
            return {"dz": np.where(y > 0, v, 0.0) if act else v}
        yield mk("gnnmp_pool_grad_act_f32", f"N{N}_D{D}_act{act}", tags,
                 [Arr("dpool", "in", dpool), Arr("graph_indicator", "in", IX(ids, ib, base)), ib, base, Arr("inv_count", "in", inv) if has_inv else None,
                  Arr("y", "in", y), act, Arr("dz", "out", shape=(N, D)), N, G, D, STREAM], ref)


# ---- softmax and attention -------------------------------------------------------------------------------------------------------
@cases_of("gnnmp_edge_softmax_f32")
def _(ctx):
    more = [(ctx.r300, 260, set())] if hasattr(ctx, "r300") else []                                        # (two feature tiles)
    for g, H, tags in list(ctx.graph_shapes(Ds=(1, 2, 3, 4, 6, 7, 100, 129), small=(3, 4), ws=(3,))) + more:
        lg = F(rng_of("edge_softmax", g.name, H), g.E, H) * f32(3)
        yield mk("gnnmp_edge_softmax_f32", f"{g.name}_H{H}", tags, [Pl(g), Arr("logits", "in", lg), Arr("alpha", "out", shape=(g.E, H)), H, STREAM],
                 lambda host, g=g, lg=lg: {"alpha": orc().softmax_edge_neighbors(g.t, g.n_dst, lg)})


@cases_of("gnnmp_segment_softmax_f32")
def _(ctx):
    from oracle import graphwise
    for k, (K, D, tags) in enumerate(row_shapes(Ds=(1, 2, 3, 4, 6, 7, 100, 129))):
        G = 1 if K == 1 else 9
        r = rng_of("segment_softmax", K, D)
        if ("seg", K) not in ctx.cache:                 # one graph per K: the wide call and the small one share its plan
            gi = rng_of("segment_graph", K).permutation(_segments(rng_of("segment_ids", K), K, G))     # an UNSORTED indicator: the plan route takes any
            ctx.cache["seg", K] = Graph(f"seg{K}", np.arange(1, K + 1), gi, K, G)
        g = ctx.cache["seg", K]
        gi = g.t
        x = F(r, K, D) * f32(3)
        den_add = float(np.finfo(f32).eps) if k % 2 else 0.0
        yield mk("gnnmp_segment_softmax_f32", f"K{K}_D{D}", tags | ({"ws"} if (K, D) == (33, 4) else set()), [Pl(g), Arr("x", "in", x), Arr("out", "out", shape=(K, D)), D, den_add, STREAM],
                 lambda host, x=x, gi=gi, G=G, den_add=den_add: {"out": graphwise._segment_softmax(x, gi, G, den_add)})


@cases_of("gnnmp_gat_node_scores_f32")
def _(ctx):
    for k, (H, C, tags) in enumerate(HC):
        for N in ((33,) if k else (1, 31, 33, 300)):
            r = rng_of("node_scores", H, C, N)
            Wx, a = F(r, N, H, C), F(r, H, 2 * C)
            which = k % 3            # both outputs, dst only, src only
            def ref(host, Wx=Wx, a=a, C=C, which=which):
                out = {}
                if which != 2:
                    out["score_dst"] = (a.astype(f64)[None, :, :C] * Wx).sum(-1)
                if which != 1:
                    out["score_src"] = (a.astype(f64)[None, :, C:] * Wx).sum(-1)
                return out
            yield mk("gnnmp_gat_node_scores_f32", f"N{N}_H{H}_C{C}_{which}", tags if N == 33 else (),
                     [Arr("Wx", "in", Wx), Arr("a", "in", a), Arr("score_dst", "out", shape=(N, H)) if which != 2 else None,
                      Arr("score_src", "out", shape=(N, H)) if which != 1 else None, N, H, C, STREAM], ref)


def lrelu(x, slope):
    return np.where(x > 0, x, slope * x)


def attn_ref(g, loops, mode, Q, K, V, a, slope, scale, H, C, bias=None, act=0, escore=None, keep=None, p=0.0, dout=None, split_dst=False):
    """float64 restatement of the one-pass attention and of its pullback (the softmax rrule written out): a dict of every array the
    forward and backward entry points produce"""
    s, t = g.s - 1, g.t - 1
    if loops:
        s, t = np.concatenate([s, np.arange(g.n)]), np.concatenate([t, np.arange(g.n)])
    nd, ns = g.n_dst, g.n_src
    Q, K, V = (np.asarray(v, f64).reshape(-1, H, C) for v in (Q, K, V))
    a = None if a is None else np.asarray(a, f64)
    Qt, Ks = Q[t], K[s]
    z = u = None
    if mode == 0:
        z = (a[None, :, :C] * Qt).sum(-1) + (a[None, :, C:] * Ks).sum(-1)
        if escore is not None:
            z = z + np.asarray(escore, f64)
        l = lrelu(z, slope)
    elif mode == 1:
        u = Qt + Ks
        l = (a[None] * lrelu(u, slope)).sum(-1)
    elif mode == 2:
        l = (Qt * Ks).sum(-1) / scale
    else:
        l = scale * (Qt * Ks).sum(-1) / (np.sqrt((Qt ** 2).sum(-1)) * np.sqrt((Ks ** 2).sum(-1)))
    m = np.full((nd, H), -np.inf)
    np.maximum.at(m, t, l)
    ex = np.exp(l - m[t])
    den = seg_sum(t, ex, nd)
    alpha = ex / den[t]
    kk = np.ones_like(alpha) if keep is None else np.asarray(keep, f64)[: len(t)] / (1.0 - p)
    ka = kk * alpha
    o = seg_sum(t, ka[..., None] * V[s], nd)
    res = {"alpha": alpha, "stats": np.stack([m, den], -1), "o": o,
           "out": act64(act, o.reshape(nd, H * C) + (0.0 if bias is None else np.asarray(bias, f64)))}
    if mode == 0:
        pos = (z > 0).astype(f64)
        res["oplus"] = seg_sum(t, (alpha * pos)[..., None] * V[s], nd).reshape(nd, H * C)
        res["pplus"] = seg_sum(t, alpha * pos, nd)
    if dout is None:
        return res
    do = np.asarray(dout, f64).reshape(nd, H, C)
    ge = kk * (do[t] * V[s]).sum(-1)
    Dm = seg_sum(t, alpha * ge, nd)
    dl = alpha * (ge - Dm[t])
    # dl is a difference of two terms that cancel exactly on a one-edge row: the scale its rounding error lives on, times the O(1) factors
    # every gradient entry multiplies it with
    big = max([1.0] + [float(np.abs(v).max()) for v in (a, Q, K) if v is not None and v.size])
    term = big * (np.abs(alpha * ge) + np.abs(alpha * Dm[t])).max(-1) if len(t) else np.zeros(0)
    row_t, row_s = np.zeros(nd), np.zeros(ns)
    np.maximum.at(row_t, t, term)                    # per destination row / per source row: the largest cancelling term among its edges
    np.maximum.at(row_s, s, term)
    res.update(gscale=float(term.max()) if len(t) else 0.0, gscale_t=row_t, gscale_s=row_s)
    dV = seg_sum(s, ka[..., None] * do[t], ns)
    if mode == 0:
        dz = dl * np.where(z > 0, 1.0, slope)
        dsd, dss = seg_sum(t, dz, nd), seg_sum(s, dz, ns)
        dsrc = dV + dss[..., None] * a[None, :, C:]
        ddst = dsd[..., None] * a[None, :, :C]
        res.update(dsd=dsd, dss=dss, da=np.concatenate([(dsd[..., None] * Q).sum(0), (dss[..., None] * K).sum(0)], -1))
        if split_dst:
            res.update(dWx_src=dsrc.reshape(ns, H * C), dWx_dst=ddst.reshape(nd, H * C))
        else:
            res.update(dWx_src=(dsrc + ddst).reshape(ns, H * C))
    elif mode == 1:
        du = dl[..., None] * a[None] * np.where(u > 0, 1.0, slope)
        res.update(dQ=seg_sum(t, du, nd).reshape(nd, H * C), dK=(seg_sum(s, du, ns) + dV).reshape(ns, H * C),
                   da=(dl[..., None] * lrelu(u, slope)).sum(0))
    elif mode == 2:
        res.update(dQ=seg_sum(t, (dl / scale)[..., None] * Ks, nd).reshape(nd, H * C), dK=seg_sum(s, (dl / scale)[..., None] * Qt, ns).reshape(ns, H * C),
                   dV=dV.reshape(ns, H * C))
    return res


ATT_HC = ((3, 7), (3, 6), (5, 4), (8, 16), (1, 1), (1, 33), (2, 8))     # (8, 16): 128 floats fit a wave only with 8- or 16-byte lanes
WIDE = ("Wx_src", "out", "oplus", "dout", "dWx_src", "Q", "K", "V", "dQ", "dK", "dV", "dA")


def att_align(H, C, base=None):
    """the statuses the header documents for an under-aligned pointer of the one-pass attention: `line` must be 16-byte aligned
    (GNNMP_EINVAL, pullbacks only); a [.][H*C] array that is under-aligned for the lane width the row needs to fit one wave is refused
    with GNNMP_EUNSUPPORTED — only possible for rows of more than 64 floats"""
    d = dict(base or {})
    if H * C > 64:
        d.update({n: EUNSUPPORTED for n in WIDE})
    return d


def att_shapes(ctx, loops):
    """(graph, H, C, tags): every head shape on the hub graph, two on the others (the edgeless graph only where the plan adds self loops
    or no statistics are written)"""
    if hasattr(ctx, "att_shapes"):                       # a context with graphs of its own (GeomCtx)
        yield from ctx.att_shapes(loops)
        return
    for k, (H, C) in enumerate(ATT_HC):
        yield ctx.hub, H, C, ({"align"} if k < 4 else set()) | ({"side", "ws"} if k == 0 else set())
    for g in (ctx.e0, ctx.one, ctx.r31, ctx.r33, ctx.r300):
        for H, C in ((3, 7), (2, 8)) + (((1, 1),) if g is ctx.r300 else ()):     # (1, 1): 64 rows to a wave, more than one block of them
            yield g, H, C, set()


def nonempty(g, loops):
    return np.ones(g.n_dst, bool) if loops else g.indeg() > 0


def _gat_forward(export, kind):
    """kind: conv | edge | stats | train | drop"""
    def build(ctx):
        loops = kind in ("stats", "drop")
        for k, (g, H, C, tags) in enumerate(att_shapes(ctx, loops)):
            r = rng_of(export, g.name, H, C)
            Wx, a = F(r, g.n, H * C), F(r, H, 2 * C)
            bias = F(r, H * C) if k % 2 == 0 else None
            act, slope, p, seed = k % 2, 0.2, 0.25, 0x1234567890ABCDEF + k
            Etot = g.E + (g.n if loops else 0)
            esc = F(r, g.E, H) if kind == "edge" else None
            keep = orc().dropout_keep(seed, p, Etot, H) if kind == "drop" else None
            def ref(host, g=g, H=H, C=C, Wx=Wx, a=a, bias=bias, act=act, esc=esc, keep=keep, loops=loops):
                R = attn_ref(g, loops, 0, Wx, Wx, Wx, a, slope, 1.0, H, C, bias, act, esc, keep, p if keep is not None else 0.0)
                ne = nonempty(g, loops)
                out = {"out": R["out"]}
                if kind in ("stats", "train", "drop"):
                    out["stats"] = E(R["stats"], rows=ne)        # an empty row's (m, den) is written, but the header gives it no value
                if kind == "train":
                    out["oplus"], out["pplus"] = R["oplus"], R["pplus"]
                return out
            args = [Pl(g, loops=loops), Arr("Wx_src", "in", Wx), None, Arr("a", "in", a)]
            if kind == "edge":
                args.append(Arr("edge_score", "in", esc))
            args.append(slope)
            if kind == "drop":
                args += [p, seed]
            args += [Arr("bias", "in", bias) if bias is not None else None, act, Arr("out", "out", shape=(g.n, H * C))]
            if kind in ("stats", "train", "drop"):
                args.append(Arr("stats", "out", shape=(g.n, H, 2)))
            if kind == "train":
                args += [Arr("oplus", "out", shape=(g.n, H * C)), Arr("pplus", "out", shape=(g.n, H))]
            yield mk(export, f"{g.name}_H{H}_C{C}", tags, args + [H, C, STREAM], ref, align_status={} if kind == "conv" else att_align(H, C))
    return build


for _kind in ("conv", "edge", "stats", "train", "drop"):
    _name = "gnnmp_gat_conv_f32" if _kind == "conv" else f"gnnmp_gat_conv_{_kind}_f32"
    TABLE[_name] = _gat_forward(_name, _kind)


@cases_of("gnnmp_gat_aggregate_f32")
def _(ctx):
    for k, (g, H, C, tags) in enumerate(att_shapes(ctx, False)):
        r = rng_of("gat_aggregate", g.name, H, C)
        Wx, sd, ss = F(r, g.n, H * C), F(r, g.n, H), F(r, g.n, H)
        bias = F(r, H * C) if k % 2 else None
        act, want_alpha = k % 2, k % 3 != 2
        def ref(host, g=g, H=H, C=C, Wx=Wx, sd=sd, ss=ss, bias=bias, act=act, want_alpha=want_alpha):
            s, t = g.s - 1, g.t - 1
            l = lrelu(sd.astype(f64)[t] + ss.astype(f64)[s], 0.2)
            m = np.full((g.n, H), -np.inf)
            np.maximum.at(m, t, l)
            ex = np.exp(l - m[t])
            alpha = ex / seg_sum(t, ex, g.n)[t]
            o = seg_sum(t, alpha[..., None] * Wx.astype(f64).reshape(-1, H, C)[s], g.n).reshape(g.n, H * C)
            out = {"out": act64(act, o + (0.0 if bias is None else bias.astype(f64)))}
            if want_alpha:
                out["alpha_out"] = alpha
            return out
        yield mk("gnnmp_gat_aggregate_f32", f"{g.name}_H{H}_C{C}", tags,
                 [Pl(g), Arr("Wx_src", "in", Wx), Arr("score_dst", "in", sd), Arr("score_src", "in", ss), 0.2, Arr("bias", "in", bias) if bias is not None else None,
                  act, Arr("out", "out", shape=(g.n, H * C)), Arr("alpha_out", "out", shape=(g.E, H)) if want_alpha else None, H, C, STREAM], ref)


def _attn_conv(export, drop):
    def build(ctx):
        for k, (g, H, C, tags) in enumerate(att_shapes(ctx, True)):
            mode = (1, 2, 3, 1)[k % 4] if not drop else 1
            if mode == 3:
                H, C = 1, H * C
            loops = True
            r = rng_of(export, g.name, H, C, mode)
            Q, K, V, a = F(r, g.n, H * C), F(r, g.n, H * C), F(r, g.n, H * C), F(r, H, C)
            sepV = mode == 2
            bias = F(r, H * C) if k % 2 == 0 else None
            act, slope, scale, p, seed = k % 2, 0.2, 1.7, 0.25, 77 + k
            keep = orc().dropout_keep(seed, p, g.E + g.n, H) if drop else None
            want_stats = k % 3 != 1
            def ref(host, g=g, H=H, C=C, mode=mode, Q=Q, K=K, V=V, a=a, bias=bias, act=act, keep=keep, sepV=sepV, want_stats=want_stats):
                R = attn_ref(g, True, mode, Q, K, V if sepV else K, a, slope, scale, H, C, bias, act, None, keep, p if keep is not None else 0.0)
                out = {"out": R["out"]}
                if want_stats:
                    out["stats"] = R["stats"]
                return out
            args = [Pl(g, loops=loops), mode, Arr("Q", "in", Q), Arr("K", "in", K), Arr("V", "in", V) if sepV else None,
                    Arr("a", "in", a) if mode == 1 else None, slope, scale]
            if drop:
                args += [p, seed]
            args += [Arr("bias", "in", bias) if bias is not None else None, act, Arr("out", "out", shape=(g.n, H * C)),
                     Arr("stats", "out", shape=(g.n, H, 2)) if want_stats else None, H, C, STREAM]
            yield mk(export, f"{g.name}_m{mode}_H{H}_C{C}", tags, args, ref, align_status=att_align(H, C))
    return build


TABLE["gnnmp_attn_conv_f32"] = _attn_conv("gnnmp_attn_conv_f32", False)
TABLE["gnnmp_attn_conv_drop_f32"] = _attn_conv("gnnmp_attn_conv_drop_f32", True)

# `line` is the one argument of the attention pullbacks the header asks 16-byte alignment for (GNNMP_EINVAL otherwise)
LINE_ALIGN = {"line": EINVAL}


def _gat_grad(export, two, drop=False):
    def build(ctx):
        for k, (g, H, C, tags) in enumerate(att_shapes(ctx, True)):
            r = rng_of(export, g.name, H, C)
            Wx, a, dout = F(r, g.n, H * C), F(r, H, 2 * C), F(r, g.n, H * C)
            bias = F(r, H * C) if k % 2 == 0 else None
            act, slope = (k % 2 if two else 0), 0.2
            p, seed = (0.25, 0xABCDEF0123 + k) if drop else (0.0, 0)
            keep = orc().dropout_keep(seed, p, g.E + g.n, H) if drop else None
            R = attn_ref(g, True, 0, Wx, Wx, Wx, a, slope, 1.0, H, C, bias, act, keep=keep, p=p, dout=dout)
            want_da = k % 3 != 1
            if two and act:                                      # dout = dL/d(o + bias): relu's switched-off entries carry 0
                dout = np.where(R["out"] > 0, dout, 0).astype(f32)
                R = attn_ref(g, True, 0, Wx, Wx, Wx, a, slope, 1.0, H, C, bias, act, keep=keep, p=p, dout=dout)
            def ref(host, R=R, want_da=want_da):
                out = {"dsd": E(R["dsd"], scale=R["gscale_t"]), "dss": E(R["dss"], scale=R["gscale_s"]),
                       "dWx_src": E(R["dWx_src"], scale=R["gscale_s"] + R["gscale_t"])}       # Wx_dst = Wx_src: both halves land in one row
                if want_da:
                    out["da"] = E(R["da"], scale=R["gscale"])
                return out
            args = [Pl(g, loops=True), Pl(g, T=True, loops=True), Arr("Wx_src", "in", Wx), None, Arr("a", "in", a), slope] + ([p, seed] if drop else [])
            args.append(Arr("stats", "in", R["stats"].astype(f32)))
            if two:
                args += [Arr("out", "in", R["out"].astype(f32)), Arr("bias", "in", bias) if bias is not None else None,
                         Arr("oplus", "in", R["oplus"].astype(f32)), Arr("pplus", "in", R["pplus"].astype(f32))]
            args += [Arr("dout", "in", dout), Arr("line", "scratch", shape=(g.n, H, 4)), Arr("dsd", "out", shape=(g.n, H)), Arr("dss", "out", shape=(g.n, H)),
                     Arr("dWx_src", "out", shape=(g.n, H * C)), None, Arr("da", "out", shape=(H, 2 * C)) if want_da else None, H, C, STREAM]
            yield mk(export, f"{g.name}_H{H}_C{C}", tags, args, ref, align_status=att_align(H, C, LINE_ALIGN))
    return build


TABLE["gnnmp_gat_conv_grad_f32"] = _gat_grad("gnnmp_gat_conv_grad_f32", False)
TABLE["gnnmp_gat_conv_grad2_f32"] = _gat_grad("gnnmp_gat_conv_grad2_f32", True)
TABLE["gnnmp_gat_conv_grad_drop_f32"] = _gat_grad("gnnmp_gat_conv_grad_drop_f32", False, drop=True)


def _attn_grad(export, drop):
    def build(ctx):
        for k, (g, H, C, tags) in enumerate(att_shapes(ctx, True)):
            mode = 1 if drop else 1 + k % 2                 # the dropped pullback exists for the GATV2 logit
            p, seed = (0.25, 0x5EED00 + k) if drop else (0.0, 0)
            keep = orc().dropout_keep(seed, p, g.E + g.n, H) if drop else None
            r = rng_of(export, g.name, H, C)
            Q, K, V, a, dout = F(r, g.n, H * C), F(r, g.n, H * C), F(r, g.n, H * C), F(r, H, C), F(r, g.n, H * C)
            slope, scale = 0.2, 1.7
            R = attn_ref(g, True, mode, Q, K, V if mode == 2 else K, a, slope, scale, H, C, keep=keep, p=p, dout=dout)
            def ref(host, R=R, mode=mode):
                out = {"dQ": E(R["dQ"], scale=R["gscale_t"]), "dK": E(R["dK"], scale=R["gscale_s"])}
                out.update({"dV": R["dV"]} if mode == 2 else {"da": E(R["da"], scale=R["gscale"])})
                return out
            yield mk(export, f"{g.name}_m{mode}_H{H}_C{C}", tags,
                     [Pl(g, loops=True), Pl(g, T=True, loops=True), mode, Arr("Q", "in", Q), Arr("K", "in", K), Arr("V", "in", V) if mode == 2 else None,
                      Arr("a", "in", a) if mode == 1 else None, slope, scale] + ([p, seed] if drop else []) + [Arr("stats", "in", R["stats"].astype(f32)), Arr("dout", "in", dout),
                      Arr("line", "scratch", shape=(g.n, H, 4)), Arr("dQ", "out", shape=(g.n, H * C)), Arr("dK", "out", shape=(g.n, H * C)),
                      Arr("dV", "out", shape=(g.n, H * C)) if mode == 2 else None, Arr("dA", "scratch", shape=(g.n, H * C)) if mode == 1 else None,
                      Arr("da", "out", shape=(H, C)) if mode == 1 else None, H, C, STREAM], ref, align_status=att_align(H, C, LINE_ALIGN))
    return build


TABLE["gnnmp_attn_conv_grad_f32"] = _attn_grad("gnnmp_attn_conv_grad_f32", False)
TABLE["gnnmp_attn_conv_grad_drop_f32"] = _attn_grad("gnnmp_attn_conv_grad_drop_f32", True)


@cases_of("gnnmp_dropout_keep_u8")
def _(ctx):
    for k, (n, H) in enumerate(((1, 1), (31, 3), (33, 4), (300, 7), (70001, 2))):
        seed, p = 0xDEADBEEF12345 + k, 0.3
        yield mk("gnnmp_dropout_keep_u8", f"n{n}_H{H}", {"align"} | ({"side"} if k == 2 else set()),
                 [seed, p, n, H, Arr("keep", "out", shape=(n, H), dtype=np.uint8), STREAM],
                 lambda host, seed=seed, n=n, H=H: {"keep": E(orc().dropout_keep(seed, p, n, H), "exact")})


# ---- dense -----------------------------------------------------------------------------------------------------------------------
def dense_guard(width):
    return 32 * 4 * int(width)            # one full store tile of the dense kernels: 32 rows of the output


@cases_of("gnnmp_dense_f32")
def _(ctx):
    shapes = [(33, 100, 0, 100, {"align", "side"}), (33, 128, 128, 128, {"align"}), (300, 100, 100, 256, {"align"}), (1, 3, 0, 5, ()), (31, 7, 6, 3, {"align"}),
              (33, 4, 0, 4, ()), (300, 16, 16, 128, ()), (33, 260, 0, 129, ()), (31, 127, 1, 2, ()), (300, 128, 0, 64, ()), (33, 2, 0, 1, ()), (300, 6, 0, 260, ())]
    for k, (N, K1, K2, Dout, tags) in enumerate(shapes):
        layout, pad = k % 2, (0, 0, 4, 3)[k % 4]               # both w_layouts; ldw larger than the row on half of the shapes
        act, has_b = k % 2, k % 3 != 0
        r = rng_of("dense", N, K1, K2, Dout)
        x1, x2 = F(r, N, K1), (F(r, N, K2) if K2 else None)
        Wf = F(r, Dout, K1 + K2) * f32(0.3)
        b = F(r, Dout) if has_b else None
        def stored(W):
            if layout == 0:
                buf = F(r, W.shape[0], W.shape[1] + pad)
                buf[:, :W.shape[1]] = W
            else:
                buf = F(r, W.shape[1], W.shape[0] + pad)
                buf[:, :W.shape[0]] = W.T
            return buf
        W1, W2 = stored(Wf[:, :K1]), (stored(Wf[:, K1:]) if K2 else None)
        def ref(host, x1=x1, x2=x2, Wf=Wf, b=b, act=act):
            xin = np.concatenate([x1, x2], 1).astype(f64) if x2 is not None else x1.astype(f64)
            pre = xin @ Wf.astype(f64).T + (0.0 if b is None else b.astype(f64))
            mag = np.abs(xin) @ np.abs(Wf.astype(f64)).T + (0.0 if b is None else np.abs(b.astype(f64)))
            return {"out": E(act64(act, pre), "mag", mag=mag)}
        yield mk("gnnmp_dense_f32", f"N{N}_K{K1}+{K2}_D{Dout}_l{layout}p{pad}", tags,
                 [Arr("x1", "in", x1), Arr("W1", "in", W1), K1, W1.shape[1], Arr("x2", "in", x2) if K2 else None, Arr("W2", "in", W2) if K2 else None, K2,
                  W2.shape[1] if K2 else 0, layout, Arr("bias", "in", b) if has_b else None, act, Arr("out", "out", shape=(N, Dout)), N, Dout, STREAM], ref,
                 guard=dense_guard(max(Dout, K1, K2)))


@cases_of("gnnmp_fused_conv_f32")
def _(ctx):
    # the header: the feature arrays must be 16-byte aligned, anything else returns GNNMP_EUNSUPPORTED.  By default the entry point also
    # refuses graphs whose aggregate fits the Infinity Cache (the unfused pair is faster there); knob 14 forces the kernel, as
    # tests/test_fused_conv.py does
    al = {n: EUNSUPPORTED for n in ("xj", "xi", "out", "agg_out")}
    shapes = ctx.fused_shapes() if hasattr(ctx, "fused_shapes") else \
             [(ctx.hub, 100, 0, 100, {"align", "side", "ws"}), (ctx.hub, 128, 0, 128, {"align"}), (ctx.hub, 64, 64, 128, {"align"}), (ctx.hub, 4, 4, 8, {"align"}), (ctx.r31, 16, 0, 32, ()),
              (ctx.r33, 100, 100, 64, ()), (ctx.r300, 64, 64, 128, ()), (ctx.r300, 100, 100, 128, ())]
    for k, (g, D, D1, Dout, tags) in enumerate(shapes):
        layout, scaled, act = k % 2, k % 2 == 0, k % 2
        aggr = SUM if scaled else (SUM, MEAN)[k % 4 // 2]
        r = rng_of("fused_conv", g.name, D, D1, Dout)
        xj, w = F(r, g.n, D), F(r, g.E)
        ss = (0.5 + r.random(g.n)).astype(f32) if scaled else None
        sd = (0.5 + r.random(g.n)).astype(f32) if scaled else None
        xi = F(r, g.n, D1) if D1 else None
        Wa, Wr, b = F(r, Dout, D) * f32(0.3), (F(r, Dout, D1) * f32(0.3) if D1 else None), F(r, Dout)
        pad = (0, 0, 4, 8)[k % 4]                       # ldw larger than the row on half of the shapes, in both layouts
        def st(W):
            M = W if layout == 0 else W.T
            buf = F(r, M.shape[0], M.shape[1] + pad)
            buf[:, :M.shape[1]] = M
            return buf
        Wr_s, Wa_s = (st(Wr) if D1 else None), st(Wa)
        def ref(host, g=g, aggr=aggr, xj=xj, w=w, ss=ss, sd=sd, xi=xi, Wa=Wa, Wr=Wr, b=b, act=act, scaled=scaled):
            A = _prop_ref(ctx, g, aggr, xj, w if scaled else None, ss, sd)
            A64 = A.value.astype(f64)
            pre = A64 @ Wa.astype(f64).T + b.astype(f64) + (xi.astype(f64) @ Wr.astype(f64).T if xi is not None else 0.0)
            return {"out": act64(act, pre), "agg_out": A}
        yield mk("gnnmp_fused_conv_f32", f"{g.name}_D{D}+{D1}_o{Dout}_l{layout}p{pad}", tags,
                 [Pl(g), aggr, Arr("xj", "in", xj), Arr("w", "in", w) if scaled else None, Arr("scale_src", "in", ss) if scaled else None, None, None,
                  Arr("scale_dst", "in", sd) if scaled else None, D, Arr("xi", "in", xi) if D1 else None, D1, Arr("W_root", "in", Wr_s) if D1 else None,
                  Wr_s.shape[1] if D1 else 0, Arr("W_agg", "in", Wa_s), Wa_s.shape[1], layout, Arr("bias", "in", b), act,
                  Arr("out", "out", shape=(g.n, Dout)), Dout, Arr("agg_out", "out", shape=(g.n, D)), STREAM], ref, guard=dense_guard(max(D, Dout)), align_status=al, knobs={14: 16})


def _grad_w_shapes():
    return [(33, 5, 16, {"align", "side"}), (300, 128, 112, {"align"}), (300, 128, 100, ()), (1, 1, 16, ()), (31, 7, 32, {"align"}), (2500, 64, 48, ()), (33, 129, 16, ())]


@cases_of("gnnmp_dense_grad_w_f32")
def _(ctx):
    from gnnmp import _lib
    for k, (N, Dout, K, tags) in enumerate(_grad_w_shapes() + [(33, 6, 3, ()), (31, 4, 127, ())]):
        r = rng_of("grad_w", N, Dout, K)
        dz, x = F(r, N, Dout), F(r, N, K)
        ws = int(_lib.load().gnnmp_dense_grad_workspace(N, Dout, K))
        which = k % 3
        def ref(host, dz=dz, x=x, which=which):
            out = {}
            if which != 2:
                out["dW"] = dz.astype(f64).T @ x.astype(f64)
            if which != 1:
                out["db"] = dz.astype(f64).sum(0)
            return out
        yield mk("gnnmp_dense_grad_w_f32", f"N{N}_o{Dout}_K{K}_{which}", tags,
                 [Arr("dz", "in", dz), Arr("x", "in", x), N, Dout, K, Arr("dW", "out", shape=(Dout, K)) if which != 2 else None,
                  Arr("db", "out", shape=(Dout,)) if which != 1 else None, Arr("workspace", "scratch", shape=(max(ws, 1),)), ws, STREAM], ref, guard=dense_guard(max(Dout, K)))


@cases_of("gnnmp_dense_grad_w2_f32")
def _(ctx):
    from gnnmp import _lib
    for N, Dout, K1, tags in _grad_w_shapes():
        K2 = (K1, 100, 4)[N % 3]
        r = rng_of("grad_w2", N, Dout, K1)
        dz, x1, x2 = F(r, N, Dout), F(r, N, K1), F(r, N, K2)
        ws = int(_lib.load().gnnmp_dense_grad_w2_workspace(N, Dout, K1, K2))
        def ref(host, dz=dz, x1=x1, x2=x2):
            d = dz.astype(f64)
            return {"out": np.concatenate([(d.T @ x1).reshape(-1), (d.T @ x2).reshape(-1), d.sum(0)])}
        yield mk("gnnmp_dense_grad_w2_f32", f"N{N}_o{Dout}_K{K1}+{K2}", tags,
                 [Arr("dz", "in", dz), Arr("x1", "in", x1), K1, Arr("x2", "in", x2), K2, N, Dout, Arr("out", "out", shape=(Dout * (K1 + K2 + 1),)),
                  Arr("workspace", "scratch", shape=(max(ws, 1),)), ws, STREAM], ref, guard=dense_guard(max(Dout, K1, K2)),
                 status=EUNSUPPORTED if K1 % 16 else OK)       # the header: K1 a multiple of 16, else GNNMP_EUNSUPPORTED


# ---- temporal --------------------------------------------------------------------------------------------------------------------
TG = ((33, 3, 5, {"align", "side"}), (1, 1, 1, ()), (31, 2, 16, {"align"}), (300, 3, 6, {"align"}), (33, 2, 128, ()), (17, 4, 100, ()))     # (N, T, out)


def tgcn_forward64(P, Uzr, Uh, h0, N, T, D):
    P, Uzr, Uh = P.astype(f64).reshape(N, T, 3 * D), Uzr.astype(f64), Uh.astype(f64)
    h = np.zeros((N, D)) if h0 is None else np.broadcast_to(h0.astype(f64), (N, D)).copy()
    y, gates = np.zeros((N, T, D)), np.zeros((N, T, 3 * D))
    for t in range(T):
        zr = sigmoid(P[:, t, :2 * D] + h @ Uzr.T)
        z, r = zr[:, :D], zr[:, D:]
        ht = np.tanh(P[:, t, 2 * D:] + (r * h) @ Uh.T)
        h = (1 - z) * h + z * ht
        y[:, t], gates[:, t] = h, np.concatenate([z, r, ht], 1)
    return y, gates


def tgcn_backward64(dy, y, gates, Uzr, Uh, h0, N, T, D):
    """backpropagation through time, the statements of the header (gnnmp_tgcn_step_grad_f32) step by step in float64, from the saved
    y and gates as given.  Returns (dP [N, T, 3D], S [N, T, 2D], dh0 [N, D])"""
    Y, G, Uz, Ur, U = y.astype(f64), gates.astype(f64), Uzr.astype(f64)[:D], Uzr.astype(f64)[D:], Uh.astype(f64)
    hstart = np.zeros((N, D)) if h0 is None else np.broadcast_to(h0.astype(f64), (N, D))
    dP, S, carry = np.zeros((N, T, 3 * D)), np.zeros((N, T, 2 * D)), np.zeros((N, D))
    for t in range(T - 1, -1, -1):
        hp = Y[:, t - 1] if t else hstart
        z, rr, ht = G[:, t, :D], G[:, t, D:2 * D], G[:, t, 2 * D:]
        dh = dy.astype(f64)[:, t] + carry
        ah = dh * z * (1 - ht * ht)
        drh = ah @ U
        az = dh * (ht - hp) * z * (1 - z)
        ar = drh * hp * rr * (1 - rr)
        carry = dh * (1 - z) + drh * rr + az @ Uz + ar @ Ur
        dP[:, t], S[:, t] = np.concatenate([az, ar, ah], 1), np.concatenate([hp, rr * hp], 1)
    return dP, S, carry


@cases_of("gnnmp_tgcn_recurrence_f32")
def _(ctx):
    for k, (N, T, D, tags) in enumerate(TG):
        r = rng_of("tgcn_rec", N, T, D)
        P, Uzr, Uh = F(r, N, T, 3 * D), F(r, 2 * D, D) * f32(0.3), F(r, D, D) * f32(0.3)
        h0 = (F(r, N, D), F(r, D), None)[k % 3]
        stride = (D, 0, 0)[k % 3]
        want_g = k % 2 == 0
        def ref(host, P=P, Uzr=Uzr, Uh=Uh, h0=h0, N=N, T=T, D=D, want_g=want_g):
            y, gates = tgcn_forward64(P, Uzr, Uh, h0, N, T, D)
            return {"y": y, "gates": gates} if want_g else {"y": y}
        yield mk("gnnmp_tgcn_recurrence_f32", f"N{N}_T{T}_D{D}", tags,
                 [Arr("P", "in", P), Arr("U_zr", "in", Uzr), Arr("U_h", "in", Uh), Arr("h0", "in", h0) if h0 is not None else None, stride,
                  Arr("y", "out", shape=(N, T, D)), Arr("gates", "out", shape=(N, T, 3 * D)) if want_g else None, N, T, D, STREAM], ref)


@cases_of("gnnmp_tgcn_recurrence_grad_f32")
def _(ctx):
    for k, (N, T, D, tags) in enumerate(TG):
        r = rng_of("tgcn_rec_grad", N, T, D)
        P, Uzr, Uh, dy = F(r, N, T, 3 * D), F(r, 2 * D, D) * f32(0.3), F(r, D, D) * f32(0.3), F(r, N, T, D)
        h0 = (F(r, N, D), F(r, D), None)[k % 3]
        stride = (D, 0, 0)[k % 3]
        y, gates = (v.astype(f32) for v in tgcn_forward64(P, Uzr, Uh, h0, N, T, D))
        want_S, want_h0 = k % 2 == 0, k % 3 != 2
        def ref(host, y=y, gates=gates, Uzr=Uzr, Uh=Uh, dy=dy, h0=h0, N=N, T=T, D=D, want_S=want_S, want_h0=want_h0):
            dP, S, carry = tgcn_backward64(dy, y, gates, Uzr, Uh, h0, N, T, D)
            out = {"dP": dP}
            if want_S:
                out["S"] = S
            if want_h0:
                out["dh0"] = carry
            return out
        yield mk("gnnmp_tgcn_recurrence_grad_f32", f"N{N}_T{T}_D{D}", tags,
                 [Arr("dy", "in", dy), Arr("y", "in", y), Arr("gates", "in", gates), Arr("U_zr", "in", Uzr), Arr("U_h", "in", Uh),
                  Arr("h0", "in", h0) if h0 is not None else None, stride, Arr("dP", "out", shape=(N, T, 3 * D)),
                  Arr("S", "out", shape=(N, T, 2 * D)) if want_S else None, Arr("dh0", "out", shape=(N, D)) if want_h0 else None, N, T, D, STREAM], ref)


@cases_of("gnnmp_tgcn_step_f32")
def _(ctx):
    for k, (N, T, D, tags) in enumerate(TG):
        phase, t = k % 2, T - 1 - (k % T)
        r = rng_of("tgcn_step", N, T, D)
        P, a, gates0, y0 = F(r, N, T, 3 * D), F(r, N, (1 if phase else 2) * D), r.random((N, T, 3 * D)).astype(f32), F(r, N, T, D)
        ldh = D + 3
        h = F(r, N, ldh) if k % 3 else None
        def ref(host, P=P, a=a, gates0=gates0, y0=y0, h=h, phase=phase, t=t, D=D, N=N):
            hv = np.zeros((N, D)) if h is None else h.astype(f64)[:, :D]
            g, y = gates0.astype(f64), y0.astype(f64)
            if phase == 0:
                zr = sigmoid(P.astype(f64)[:, t, :2 * D] + a)
                g[:, t, :2 * D] = zr
                return {"gates": g, "hout": zr[:, D:] * hv}
            ht = np.tanh(P.astype(f64)[:, t, 2 * D:] + a)
            z = g[:, t, :D]
            g[:, t, 2 * D:] = ht
            hn = (1 - z) * hv + z * ht
            y[:, t] = hn
            return {"gates": g, "hout": hn, "y": y}
        yield mk("gnnmp_tgcn_step_f32", f"N{N}_T{T}_D{D}_p{phase}", tags,
                 [phase, Arr("P", "in", P), Arr("a", "in", a), Arr("h", "in", h) if h is not None else None, ldh, Arr("gates", "inout", gates0),
                  Arr("hout", "out", shape=(N, D)), Arr("y", "inout", y0) if phase else None, N, T, t, D, STREAM], ref)


@cases_of("gnnmp_tgcn_step_grad_f32")
def _(ctx):
    for k, (N, T, D, tags) in enumerate(TG):
        phase, t = k % 2, k % T
        r = rng_of("tgcn_step_grad", N, T, D)
        dy, carry, gates, drh = F(r, N, T, D), F(r, N, D), r.random((N, T, 3 * D)).astype(f32) * f32(0.9), F(r, N, D)
        ldh = D + 1
        h = F(r, N, ldh)
        dP0, dzr0, part0, S0, dah0 = F(r, N, T, 3 * D), F(r, N, 2 * D), F(r, N, D), F(r, N, T, 2 * D), F(r, N, D)
        has_c, has_S = k % 3 != 0, k % 4 != 3
        def ref(host, dy=dy, carry=carry, gates=gates, drh=drh, h=h, dP0=dP0, dzr0=dzr0, part0=part0, S0=S0, phase=phase, t=t, D=D, has_c=has_c, has_S=has_S):
            G, hp = gates.astype(f64)[:, t], h.astype(f64)[:, :D]
            z, rr, ht = G[:, :D], G[:, D:2 * D], G[:, 2 * D:]
            dP, dzr, part, S = dP0.astype(f64), dzr0.astype(f64), part0.astype(f64), S0.astype(f64)
            if phase == 0:
                gq = dy.astype(f64)[:, t] + (carry if has_c else 0.0)
                ah, az = gq * z * (1 - ht * ht), gq * (ht - hp) * z * (1 - z)
                dP[:, t, :D], dP[:, t, 2 * D:], dzr[:, :D] = az, ah, az
                return {"dP": dP, "dah": ah, "dzr": dzr, "part": gq * (1 - z)}
            ar = drh.astype(f64) * hp * rr * (1 - rr)
            dP[:, t, D:2 * D], dzr[:, D:] = ar, ar
            out = {"dP": dP, "dzr": dzr, "part": part + drh.astype(f64) * rr}
            if has_S:
                S[:, t, :D], S[:, t, D:] = hp, rr * hp
                out["S"] = S
            return out
        args = [phase, Arr("dy", "in", dy), Arr("carry", "in", carry) if has_c and phase == 0 else None, Arr("gates", "in", gates), Arr("h", "in", h), ldh,
                Arr("drh", "in", drh) if phase else None, Arr("dP", "inout", dP0), Arr("dah", "out", shape=(N, D)) if phase == 0 else Arr("dah", "scratch", shape=(N, D)),
                Arr("dzr", "inout", dzr0), Arr("part", "inout", part0), Arr("S", "inout", S0) if has_S and phase else None, N, T, t, D, STREAM]
        yield mk("gnnmp_tgcn_step_grad_f32", f"N{N}_T{T}_D{D}_p{phase}", tags, args, ref)


# ---- graph prep with caller-owned outputs ------------------------------------------------------------------------------------------
PREP = ((1, 2), (31, 90), (33, 100), (300, 900), (40, 0))


@cases_of("gnnmp_add_self_loops")
def _(ctx):
    for k, (n, E_) in enumerate(PREP):
        ib, base = IDX[k % 4]
        r = rng_of("asl", n, E_)
        s1, t1 = r.integers(1, n + 1, E_), r.integers(1, n + 1, E_)
        w = F(r, E_) if k % 2 == 0 else None
        def ref(host, s1=s1, t1=t1, n=n, w=w, ib=ib, base=base):
            s2, t2, w2 = orc().add_self_loops(s1, t1, n, w)
            out = {"out_src": E(IX(s2, ib, base), "exact"), "out_dst": E(IX(t2, ib, base), "exact")}
            if w is not None:
                out["out_w"] = E(w2, "exact")
            return out
        dt = np.int64 if ib == 8 else np.int32
        yield mk("gnnmp_add_self_loops", f"n{n}_E{E_}_i{ib}b{base}", {"align"} | ({"side"} if k == 2 else set()),
                 [Arr("src", "in", IX(s1, ib, base)), Arr("dst", "in", IX(t1, ib, base)), ib, base, E_, n, Arr("out_src", "out", shape=(E_ + n,), dtype=dt),
                  Arr("out_dst", "out", shape=(E_ + n,), dtype=dt), Arr("w", "in", w) if w is not None else None,
                  Arr("out_w", "out", shape=(E_ + n,)) if w is not None else None, STREAM], ref)


@cases_of("gnnmp_batch_coo")
def _(ctx):
    for k, sizes in enumerate(((1,), (5, 0, 7, 19), (33, 31, 1, 64, 2), (300, 5))):
        ib, base = IDX[k % 4]
        r = rng_of("batch", sizes)
        graphs = [(r.integers(1, n + 1, 3 * n), r.integers(1, n + 1, 3 * n), n) if n else (np.zeros(0, np.int64), np.zeros(0, np.int64), 0) for n in sizes]
        s2, t2, gi, N = orc().batch(graphs)
        ep = np.array([0] + [len(g[0]) for g in graphs], np.int64).cumsum()
        npt = np.array([0] + [g[2] for g in graphs], np.int64).cumsum()
        s = np.concatenate([g[0] for g in graphs])
        t = np.concatenate([g[1] for g in graphs])
        dt = np.int64 if ib == 8 else np.int32
        yield mk("gnnmp_batch_coo", f"G{len(sizes)}_N{N}_i{ib}b{base}", {"align"} | ({"side"} if k == 1 else set()),
                 [Arr("src", "in", IX(s, ib, base)), Arr("dst", "in", IX(t, ib, base)), ib, base, Arr("edge_ptr", "in", ep), Arr("node_ptr", "in", npt), len(sizes),
                  Arr("out_src", "out", shape=(len(s),), dtype=dt), Arr("out_dst", "out", shape=(len(s),), dtype=dt), Arr("graph_indicator", "out", shape=(N,), dtype=dt), STREAM],
                 lambda host, s2=s2, t2=t2, gi=gi, ib=ib, base=base: {"out_src": E(IX(s2, ib, base), "exact"), "out_dst": E(IX(t2, ib, base), "exact"),
                                                                      "graph_indicator": E(IX(gi, ib, base), "exact")})


@cases_of("gnnmp_sort_edge_index")
def _(ctx):
    for k, (n, E_) in enumerate(PREP[:4] + ((500, 5000),)):
        ib, base = IDX[k % 4]
        r = rng_of("sort", n, E_)
        u, v = r.integers(1, n + 1, E_), r.integers(1, n + 1, E_)
        o = np.lexsort((v, u))
        dt = np.int64 if ib == 8 else np.int32
        yield mk("gnnmp_sort_edge_index", f"n{n}_E{E_}_i{ib}b{base}", {"align"} | ({"side"} if k == 2 else set()),
                 [Arr("u", "in", IX(u, ib, base)), Arr("v", "in", IX(v, ib, base)), ib, base, E_, Arr("u_out", "out", shape=(E_,), dtype=dt),
                  Arr("v_out", "out", shape=(E_,), dtype=dt), STREAM],
                 lambda host, u=u, v=v, o=o, ib=ib, base=base: {"u_out": E(IX(u[o], ib, base), "exact"), "v_out": E(IX(v[o], ib, base), "exact")})


@cases_of("gnnmp_unique_append")
def _(ctx):
    for k, (n, nc) in enumerate(((1, 1), (31, 50), (33, 100), (300, 900))):
        ib, base = IDX[k % 4]
        r = rng_of("unique", n, nc)
        present = r.permutation(n)[: n // 3] + 1                    # the set so far, in list order
        map0 = np.zeros(n, np.int32)
        map0[present - 1] = np.arange(1, len(present) + 1)
        cand = r.integers(1, n + 1, nc)
        seen, new = set(present.tolist()), []
        for c in cand.tolist():
            if c not in seen:
                seen.add(c)
                new.append(c)
        map1 = map0.copy()
        map1[np.asarray(new, np.int64) - 1] = len(present) + np.arange(1, len(new) + 1)
        dt = np.int64 if ib == 8 else np.int32
        def ref(host, new=new, map1=map1, ib=ib, base=base):
            assert host["n_new"] == len(new), (host["n_new"], len(new))
            return {"map": E(map1, "exact"), "list_out": E(IX(np.asarray(new, np.int64), ib, base), "exact", prefix=len(new))}
        yield mk("gnnmp_unique_append", f"n{n}_c{nc}_i{ib}b{base}", {"align"} | ({"side"} if k == 2 else set()),
                 [Arr("map", "inout", map0), Arr("first", "scratch", shape=(n,), dtype=np.int32), n, Arr("cand", "in", IX(cand, ib, base)), ib, base, nc, len(present),
                  Arr("list_out", "out", shape=(nc,), dtype=dt), HostOut("n_new"), STREAM], ref)


@cases_of("gnnmp_induced_subgraph")
def _(ctx):
    for k, g in enumerate((ctx.hub, ctx.one, ctx.r31, ctx.r33, ctx.r300)):
        ib, base = IDX[k % 4]
        r = rng_of("induced", g.name)
        nodes = r.permutation(g.n)[: max(1, g.n // 2)] + 1
        mp = np.zeros(g.n, np.int32)
        mp[nodes - 1] = np.arange(1, len(nodes) + 1)
        so, to, eo, offs = [], [], [], [0]
        for pos, v in enumerate(nodes.tolist()):
            for e in np.flatnonzero(g.t == v).tolist():
                if mp[g.s[e] - 1]:
                    so.append(int(mp[g.s[e] - 1]))
                    to.append(pos + 1)
                    eo.append(e + 1)
            offs.append(len(so))
        tot = len(so)
        dt = np.int64 if ib == 8 else np.int32
        def ref(host, so=so, to=to, eo=eo, offs=offs, tot=tot, ib=ib, base=base):
            assert host["total"] == tot, (host["total"], tot)
            I = lambda v: E(IX(np.asarray(v, np.int64), ib, base), "exact")
            return {"offsets": E(np.asarray(offs, np.int64), "exact"), "s_out": I(so), "t_out": I(to), "eid_out": I(eo)}
        yield mk("gnnmp_induced_subgraph", f"{g.name}_i{ib}b{base}", ({"align", "side", "ws"} if g is ctx.hub else ()),
                 [Pl(g), Arr("map", "in", mp), Arr("nodes", "in", IX(nodes, ib, base)), ib, base, len(nodes), Arr("offsets", "out", shape=(len(nodes) + 1,), dtype=np.int64),
                  Arr("s_out", "out", shape=(tot,), dtype=dt), Arr("t_out", "out", shape=(tot,), dtype=dt), Arr("eid_out", "out", shape=(tot,), dtype=dt), tot,
                  HostOut("total"), STREAM], ref)


@cases_of("gnnmp_rand_edge_split")
def _(ctx):
    for k, (n, E_) in enumerate(PREP[:4]):
        ib, base = IDX[k % 4]
        r = rng_of("split", n, E_)
        s1, t1 = r.integers(1, n + 1, E_), r.integers(1, n + 1, E_)
        size1 = int(round(E_ * 0.3))
        code = (s1 - 1 + base).astype(np.int64) * (n + 2) + (t1 - 1 + base)
        def ref(host, code=code, size1=size1, n=n):
            got = {}
            def part(name):
                def pred(v, name=name):
                    got[name] = v.astype(np.int64)
                    if len(got) == 4:            # the four outputs together are a permutation of the edge list (exact integers)
                        c = np.concatenate([got["s1"] * (n + 2) + got["t1"], got["s2"] * (n + 2) + got["t2"]])
                        if not np.array_equal(np.sort(c), np.sort(code)):
                            return "the two parts are not a partition of the edges"
                    return None
                return E(pred=pred)
            return {nm: part(nm) for nm in ("s1", "t1", "s2", "t2")}
        dt = np.int64 if ib == 8 else np.int32
        yield mk("gnnmp_rand_edge_split", f"n{n}_E{E_}_i{ib}b{base}", {"align"} | ({"side"} if k == 2 else set()),
                 [Arr("s", "in", IX(s1, ib, base)), Arr("t", "in", IX(t1, ib, base)), ib, base, E_, 0, size1, 12345 + k, Arr("s1", "out", shape=(size1,), dtype=dt),
                  Arr("t1", "out", shape=(size1,), dtype=dt), Arr("s2", "out", shape=(E_ - size1,), dtype=dt), Arr("t2", "out", shape=(E_ - size1,), dtype=dt), STREAM], ref)


# ---- exports that take a record ----------------------------------------------------------------------------------------------------
# `const gnnmp_<x>_t *job` is a const HOST structure; what its non-const pointer fields point at is written.  The references are the
# float64 / exact restatements of tests/*_ref.py that each family's own test file uses (imported, not restated); the operands are drawn
# here, through rng_of, so that variant 1 of a case is the same call on other values.
def _mod(name):
    import importlib
    return importlib.import_module(name)


def part_E(init, mask, value, exact=None, **kw):
    """an in-out buffer of which the call owes only the elements of `mask` (step t of a [N][T][..] history, a column block of a panel):
    they are compared with `value` (the caller fills them with NaN, so one that was not written is not finite), every other element must
    keep the bits of `init`.  exact: the owed elements that are documented exact values (zeros of a NULL state)"""
    mask = np.broadcast_to(mask, init.shape).copy()
    kept = np.ascontiguousarray(init).view(np.uint32)[~mask].copy()

    def pred(got):
        return None if np.array_equal(np.ascontiguousarray(got).view(np.uint32)[~mask], kept) else "an element outside the part the call writes changed"
    return E(np.where(mask, value, 0.0), rows=mask, pred=pred, exact_rows=None if exact is None else np.broadcast_to(exact, init.shape)[mask], **kw)


def _hist(r, shape, t, cols=slice(None), given=None):
    """a [N][T][W] history: random everywhere, step t's `cols` NaN (to be written) or `given`; returns (array, mask of step t's cols)"""
    a = F(r, *shape)
    m = np.zeros(shape, bool)
    m[:, t, cols] = True
    a[m] = np.nan if given is None else np.asarray(given, f32).reshape(-1)
    return a, m


def _strided(r, name, role, N, D, ld, off, key=None, block=None):
    """rows of D floats with stride ld starting `off` floats into a buffer [N][ld] of its own: (buffer Arr, view Arr, mask of the block).
    block: the values of the block (else random for an input, NaN for an output)"""
    buf = F(r, N, ld)
    m = np.zeros((N, ld), bool)
    m[:, off:off + D] = True
    if block is not None:
        buf[m] = np.asarray(block, f32).reshape(-1)
    elif role != "in":
        buf[m] = np.nan
    base = Arr(key or name + "_buf", "in" if role == "in" else "inout", buf)
    return base, Arr(name, role, base=base, offset=off), m


GATE_NS, GATE_T, GATE_TS, GATE_DS = (1, 37, 300), 3, (0, 2), (1, 5, 6, 8, 260)
GATE_ALIGN = ((37, 5), (37, 6), (37, 8))


def _gate_shapes():
    """(k, N, D, t, state kind, rep, flag, tags): every (N, D); t, the kind of state, rep and the optional fields rotate so that every
    pair of them occurs"""
    k = 0
    for N in GATE_NS:
        for D in GATE_DS:
            tags = ({"align"} if (N, D) in GATE_ALIGN else set()) | ({"side"} if k == 0 else set())
            yield k, N, D, GATE_TS[(k // 2) % 2], ("mat", "vec", "null")[k % 3], 1 + k % 2, (k // 3) % 2 == 0, tags
            k += 1


def _gate_ops(r, N, D, G):
    """the operands of tests/recurrent_ref.py: gate_case, drawn from the case's generator"""
    T = GATE_T
    return dict(P=F(r, N, T, G * D), a=F(r, N, G * D), h=F(r, N, D), hvec=F(r, D), dy=F(r, N, T, D), carry=F(r, N, D), carry2=F(r, N, 2 * D),
                drh=F(r, N, 2 * D), carry_c=F(r, N, D), w=(0.5 * F(r, 4, D)).astype(f32), cnew_in=F(r, N, T, D))


def _state(r, ops, kind, N, D, name):
    """(extra slab arrays, the field's value, stride): [N][D] inside a wider buffer at an odd column, one vector, NULL"""
    if kind == "null":
        return None, 0
    if kind == "vec":
        return Arr(name, "in", ops["hvec"]), 0
    base, view, _ = _strided(r, name, "in", N, D, 2 * D + 3, 3, block=ops["h"])
    return view, 2 * D + 3


@cases_of("gnnmp_gru_cell_f32")
def _(ctx):
    RR = _mod("recurrent_ref")
    for k, N, D, t, hk, rep, flag, tags in _gate_shapes():
        for phase in (0, 1):
            r = rng_of("gru_cell", N, D, phase)
            ops = _gate_ops(r, N, D, 3)
            T = GATE_T
            f = RR.gru_forward(ops, hk, t)
            h, ldh = _state(r, ops, hk, N, D, "h")
            ldo = rep * D + 5
            want_hout = phase == 0 or flag
            hb, hv, hm = _strided(r, "hout", "out", N, rep * D, ldo, 2)
            if phase == 0:
                a = ops["a"][:, :2 * D]
                gates, gm = _hist(r, (N, T, 3 * D), t, slice(0, 2 * D))
                y = None
            else:
                a = ops["a"][:, 2 * D:]
                gates, gm = _hist(r, (N, T, 3 * D), t, slice(2 * D, 3 * D))
                gates[:, t, D:2 * D] = f["z"]                    # phase 1 reads z where phase 0 left it
                yinit, ym = _hist(r, (N, T, D), t)
                y = Arr("y", "inout", yinit)

            def ref(host, f=f, phase=phase, gates=gates, gm=gm, hb=hb, hm=hm, rep=rep, hk=hk, y=y, t=t, D=D, want_hout=want_hout):
                g = np.zeros(gates.shape)
                if phase == 0:
                    g[:, t, :D], g[:, t, D:2 * D] = f["r"], f["z"]
                    block = np.tile(f["rh"], (1, rep))
                else:
                    g[:, t, 2 * D:] = f["c"]
                    block = np.tile(f["hn"], (1, rep))
                out = {"gates": part_E(gates, gm, g)}
                if want_hout:
                    full = np.zeros(hb.data.shape)
                    full[hm] = block.reshape(-1)
                    out["hout_buf"] = part_E(hb.data, hm, full, exact=(hm if phase == 0 and hk == "null" else None))      # r * 0: an exact zero
                if phase == 1:
                    yy = np.zeros(y.data.shape)
                    yy[:, t] = f["hn"]
                    out["y"] = part_E(y.data, np.isnan(y.data), yy)
                return out
            job = Rec("gnnmp_gru_cell_t", P=Arr("P", "in", ops["P"]), a=Arr("a", "in", a), h=h, ldh=ldh, gates=Arr("gates", "inout", gates),
                      hout=hv if want_hout else None, ldhout=ldo, rep=rep, y=y)
            yield mk("gnnmp_gru_cell_f32", f"N{N}_D{D}_t{t}_{hk}_rep{rep}_p{phase}{'' if want_hout else '_nohout'}", tags if phase == 0 else tags - {"side"},
                     [phase, job, N, T, t, D, STREAM], ref, no_warmup=True)


@cases_of("gnnmp_gru_cell_grad_f32")
def _(ctx):
    RR = _mod("recurrent_ref")
    for k, N, D, t, hk, rep, flag, tags in _gate_shapes():
        for phase in (1, 0):
            r = rng_of("gru_cell_grad", N, D, phase)
            ops = _gate_ops(r, N, D, 3)
            T = GATE_T
            carries = ((True, True), (False, False), (False, True), (True, False))[k % 4]
            b = RR.gru_backward(ops, hk, t, rep, carries)
            gates = F(r, N, T, 3 * D)
            gates[:, t] = np.concatenate([b["r"], b["z"], b["c"]], 1)                 # what the forward kept
            h, ldh = _state(r, ops, hk, N, D, "h")
            ld2 = 2 * D + 1
            zero_r = hk == "null"                                                        # h = 0: dr_pre is an exact zero
            if phase == 1:
                _, c2, _ = _strided(r, "carry2", "in", N, rep * D, ld2, 1, block=ops["carry2"][:, :rep * D])
                dP, pm = _hist(r, (N, T, 3 * D), t, slice(D, 3 * D))
                darz = F(r, N, 2 * D)
                darz[:, D:] = np.nan
                job = Rec("gnnmp_gru_cell_grad_t", dy=Arr("dy", "in", ops["dy"]), carry=Arr("carry", "in", ops["carry"]) if carries[0] else None,
                          carry2=c2 if carries[1] else None, ldc2=ld2, gates=Arr("gates", "in", gates), h=h, ldh=ldh, drh=None, lddrh=ld2, rep=rep,
                          dP=Arr("dP", "inout", dP), dac=Arr("dac", "out", shape=(N, D)), darz=Arr("darz", "inout", darz), part=Arr("part", "out", shape=(N, D)))

                def ref(host, b=b, dP=dP, pm=pm, darz=darz, t=t, D=D):
                    p = np.zeros(dP.shape)
                    p[:, t, D:2 * D], p[:, t, 2 * D:] = b["dz"], b["dc"]
                    return {"dP": part_E(dP, pm, p), "dac": b["dc"], "darz": part_E(darz, np.isnan(darz), np.concatenate([b["dz"], b["dz"]], 1)),
                            "part": b["part1"]}
            else:
                _, dv, _ = _strided(r, "drh", "in", N, rep * D, ld2, 1, block=ops["drh"][:, :rep * D])
                dP, pm = _hist(r, (N, T, 3 * D), t, slice(0, D))
                darz = F(r, N, 2 * D)
                darz[:, :D] = np.nan
                part0 = F(r, N, D)
                job = Rec("gnnmp_gru_cell_grad_t", dy=None, carry=None, carry2=None, ldc2=0, gates=Arr("gates", "in", gates), h=h, ldh=ldh, drh=dv,
                          lddrh=ld2, rep=rep, dP=Arr("dP", "inout", dP), dac=None, darz=Arr("darz", "inout", darz), part=Arr("part", "inout", part0))

                def ref(host, b=b, dP=dP, pm=pm, darz=darz, part0=part0, t=t, D=D, zero_r=zero_r):
                    p = np.zeros(dP.shape)
                    p[:, t, :D] = b["dr"]
                    am = np.isnan(darz)
                    return {"dP": part_E(dP, pm, p, exact=pm if zero_r else None),
                            "darz": part_E(darz, am, np.concatenate([b["dr"], b["dr"]], 1), exact=am if zero_r else None),
                            "part": part0.astype(f64) + (b["part"] - b["part1"])}
            yield mk("gnnmp_gru_cell_grad_f32", f"N{N}_D{D}_t{t}_{hk}_rep{rep}_p{phase}_c{int(carries[0])}{int(carries[1])}", tags if phase == 1 else tags - {"side"},
                     [phase, job, N, T, t, D, STREAM], ref, no_warmup=True)


@cases_of("gnnmp_lstm_cell_f32")
def _(ctx):
    RR = _mod("recurrent_ref")
    for k, N, D, t, ck, rep, flag, tags in _gate_shapes():
        r = rng_of("lstm_cell", N, D)
        ops = _gate_ops(r, N, D, 4)
        T = GATE_T
        f = RR.lstm_forward(ops, ck, t)
        c, ldc = _state(r, ops, ck, N, D, "c")
        hb, hv, hm = _strided(r, "hout", "out", N, D, D + 5, 2)
        gates, gm = _hist(r, (N, T, 4 * D), t)
        cnew, cm = _hist(r, (N, T, D), t)
        y, ym = _hist(r, (N, T, D), t)

        def ref(host, f=f, gates=gates, gm=gm, cnew=cnew, cm=cm, y=y, ym=ym, hb=hb, hm=hm, t=t, flag=flag):
            g, cn, yy = np.zeros(gates.shape), np.zeros(cnew.shape), np.zeros(y.shape)
            g[:, t], cn[:, t], yy[:, t] = np.concatenate([f["i"], f["f"], f["g"], f["o"]], 1), f["cn"], f["hn"]
            out = {"gates": part_E(gates, gm, g), "cnew": part_E(cnew, cm, cn), "y": part_E(y, ym, yy)}
            if flag:
                full = np.zeros(hb.data.shape)
                full[hm] = f["hn"].reshape(-1)
                out["hout_buf"] = part_E(hb.data, hm, full)
            return out
        job = Rec("gnnmp_lstm_cell_t", P=Arr("P", "in", ops["P"]), a=Arr("a", "in", ops["a"]), w=Arr("w", "in", ops["w"]), c=c, ldc=ldc,
                  gates=Arr("gates", "inout", gates), cnew=Arr("cnew", "inout", cnew), hout=hv if flag else None, ldhout=D + 5, y=Arr("y", "inout", y))
        yield mk("gnnmp_lstm_cell_f32", f"N{N}_D{D}_t{t}_{ck}{'' if flag else '_nohout'}", tags, [job, N, T, t, D, STREAM], ref, no_warmup=True)


@cases_of("gnnmp_lstm_cell_grad_f32")
def _(ctx):
    RR = _mod("recurrent_ref")
    for k, N, D, t, ck, rep, flag, tags in _gate_shapes():
        r = rng_of("lstm_cell_grad", N, D)
        ops = _gate_ops(r, N, D, 4)
        T = GATE_T
        carries = ((True, True), (False, False), (True, False), (False, True))[k % 4]
        b = RR.lstm_backward(ops, ck, t, carries)
        gates, cnew = F(r, N, T, 4 * D), F(r, N, T, D)
        gates[:, t], cnew[:, t] = np.concatenate([b["i"], b["f"], b["g"], b["o"]], 1), b["cn"]          # what the forward kept
        c, ldc = _state(r, ops, ck, N, D, "c")
        _, chv, _ = _strided(r, "carry_h", "in", N, D, D + 3, 1, block=ops["carry"])
        dP, pm = _hist(r, (N, T, 4 * D), t)
        peep, qm = _hist(r, (N, T, 4 * D), t)

        def ref(host, b=b, dP=dP, pm=pm, peep=peep, qm=qm, t=t, D=D, ck=ck, flag=flag):
            p, q = np.zeros(dP.shape), np.zeros(peep.shape)
            p[:, t], q[:, t] = b["da"], b["peep"]
            out = {"dP": part_E(dP, pm, p), "da": b["da"], "dc": b["dc"]}
            if flag:
                zero = np.zeros(peep.shape, bool)
                zero[:, t, :3 * D] = ck == "null"                       # c = 0: the first three products are exact zeros
                out["peep"] = part_E(peep, qm, q, exact=zero if ck == "null" else None)
            return out
        job = Rec("gnnmp_lstm_cell_grad_t", dy=Arr("dy", "in", ops["dy"]), carry_h=chv if carries[0] else None, ldch=D + 3,
                  carry_c=Arr("carry_c", "in", ops["carry_c"]) if carries[1] else None, gates=Arr("gates", "in", gates), w=Arr("w", "in", ops["w"]), c=c,
                  ldc=ldc, cnew=Arr("cnew", "in", cnew), dP=Arr("dP", "inout", dP), da=Arr("da", "out", shape=(N, 4 * D)), dc=Arr("dc", "out", shape=(N, D)),
                  peep=Arr("peep", "inout", peep) if flag else None)
        yield mk("gnnmp_lstm_cell_grad_f32", f"N{N}_D{D}_t{t}_{ck}_c{int(carries[0])}{int(carries[1])}{'' if flag else '_nopeep'}", tags,
                 [job, N, T, t, D, STREAM], ref, no_warmup=True)


# the hop: every combination class of its nullable factors and terms (tests/test_recurrent_layers.py: HOP_COMBOS), in the order
# (w_slot, ss_slot, scale_dst, self, prev, add)
HOP_COMBOS = ((True,) * 6, (False,) * 6, (True, False, True, False, True, False), (False, True, False, True, False, True),
              (True, True, False, True, True, False), (False, False, True, False, False, True))
HOP_DS = (1, 3, 6, 8, 129, 260)      # 4-byte lanes (odd), 8-byte (% 2), 16-byte (% 4); a second feature tile at 4-byte (129) and at 16-byte lanes (260)


def _hop_operands(r, g, T, D, combo):
    """(s0, t0, operands in float32, slot order) of a hop over the plan (T: the transposed plan) of g"""
    s0, t0 = ((g.t, g.s) if T else (g.s, g.t))
    s0, t0 = s0 - 1, t0 - 1
    n_src, n_dst = (g.n_dst, g.n_src) if T else (g.n_src, g.n_dst)
    on = dict(zip(("w", "ss", "sd", "self_", "prev", "add"), combo))
    ops = dict(z=F(r, n_src, D), w=(1.0 + 0.5 * F(r, g.E)).astype(f32), ss=(1.0 + 0.5 * F(r, g.E)).astype(f32), sd=(1.0 + 0.5 * F(r, n_dst)).astype(f32),
               self_=F(r, n_dst, D), prev=F(r, n_dst, D), add=F(r, n_dst, D))
    return s0, t0, n_dst, {k: v for k, v in ops.items() if k == "z" or on[k]}, np.argsort(t0, kind="stable")


def _hop_ref(s0, t0, n_dst, ops, coef):
    R = _mod("poly_conv_ref")
    kw = {k: v.astype(f64) for k, v in ops.items() if k != "z"}
    return R.hop(s0, t0, n_dst, ops["z"].astype(f64), alpha=coef[0], beta=coef[1], gam=coef[2], **kw)


def _hop_coef(ops):
    R = _mod("poly_conv_ref")
    return R.ALPHA, R.BETA if "self_" in ops else 0.0, R.GAMMA if "prev" in ops else 0.0


@cases_of("gnnmp_poly_hop_f32")
def _(ctx):
    for k, (g, D, tags) in enumerate(ctx.graph_shapes(HOP_DS, small=(3, 8), align=(3, 6, 8), ws=(8,), rows300=(1, 260))):
        T = k % 2 == 1
        combo = HOP_COMBOS[k % 6]
        r = rng_of("poly_hop", g.name, D)
        s0, t0, n_dst, ops, order = _hop_operands(r, g, T, D, combo)
        coef = _hop_coef(ops)
        alias = {3: "prev", 4: "add"}.get(k % 5)                   # out MAY BE prev OR add
        alias = alias if alias in ops else None
        A_ = lambda nm, key, v: Arr(nm, "in", v) if key in ops else None      # noqa: E731
        f = dict(z=Arr("z", "in", ops["z"]), w_slot=A_("w_slot", "w", ops.get("w", np.zeros(0))[order] if "w" in ops else None),
                 ss_slot=A_("ss_slot", "ss", ops["ss"][order] if "ss" in ops else None), scale_dst=A_("scale_dst", "sd", ops.get("sd")),
                 self=A_("self", "self_", ops.get("self_")), prev=A_("prev", "prev", ops.get("prev")), add=A_("add", "add", ops.get("add")))
        out = Arr("out", "out", shape=(n_dst, D))
        name = "out"
        if alias:
            both = Arr(alias + "_out", "inout", ops[alias])
            f[alias], out, name = Arr(alias, "in", base=both), Arr("out", "out", base=both), alias + "_out"
        ref = lambda host, a=(s0, t0, n_dst, ops, coef), name=name: {name: _hop_ref(*a)}
        job = Rec("gnnmp_poly_hop_t", **f, alpha=coef[0], beta=coef[1], gamma=coef[2], out=out)
        yield mk("gnnmp_poly_hop_f32", f"{g.name}_D{D}_{'T' if T else 'P'}_c{k % 6}{'_out_is_' + alias if alias else ''}", tags,
                 [Pl(g, T=T), job, D, STREAM], ref, no_warmup=True)


def _ld_modes(D):
    """row strides in floats: D itself; odd (4-byte lanes whatever D is); a multiple of 2 and not of 4 (8-byte lanes at most); of 4"""
    odd = (D + 1) | 1
    two = D + 1
    while two % 4 != 2:
        two += 1
    return {"ldD": D, "odd": odd, "ld8": two, "ld16": (D + 4) // 4 * 4}


@cases_of("gnnmp_poly_hop_ld_f32")
def _(ctx):
    # 1. every operand in a buffer of its own with its own stride: each can be shifted alone (the lane width is decided over every given
    #    pointer AND every given stride)
    shapes = [(g, D, set(tags), ("ldD", "odd", "ld8", "ld16")[k % 4]) for k, (g, D, tags) in
              enumerate(ctx.graph_shapes((1, 3, 6, 8, 260), small=(6,), align=(), ws=(8,), rows300=(1,)))]
    shapes += [(ctx.hub, 8, {"align"}, "ld8"), (ctx.hub, 8, {"align"}, "ld16"), (ctx.hub, 6, {"align"}, "ld8"), (ctx.hub, 6, set(), "odd"),
               (ctx.hub, 8, set(), "odd"), (ctx.r300, 260, set(), "ld8")]
    for k, (g, D, tags, mode) in enumerate(shapes):
        T = k % 2 == 1
        combo = HOP_COMBOS[k % 6]
        r = rng_of("poly_hop_ld", g.name, D, mode)
        s0, t0, n_dst, ops, order = _hop_operands(r, g, T, D, combo)
        coef = _hop_coef(ops)
        ld = _ld_modes(D)[mode]
        lds = {"z": ld, "self": D if k % 3 == 0 else ld, "prev": ld, "add": _ld_modes(D)["ld16"] if k % 3 == 1 else ld, "out": ld}      # the strides of one call need not agree
        f, held = {}, {}
        for nm, key in (("z", "z"), ("self", "self_"), ("prev", "prev"), ("add", "add")):
            if key in ops:
                n_rows = ops[key].shape[0]
                held[nm] = _strided(r, nm, "in", n_rows, D, lds[nm], 0, block=ops[key])
            else:
                F(r, n_dst, lds[nm])                                # the draws stay in step
            f[nm] = held[nm][1] if nm in held else None
        ob, ov, om = _strided(r, "out", "out", n_dst, D, lds["out"], 0)

        def ref(host, a=(s0, t0, n_dst, ops, coef), ob=ob, om=om):
            full = np.zeros(ob.data.shape)
            full[om] = _hop_ref(*a).reshape(-1)
            return {"out_buf": part_E(ob.data, om, full)}
        job = Rec("gnnmp_poly_hop_ld_t", z=f["z"], w_slot=Arr("w_slot", "in", ops["w"][order]) if "w" in ops else None,
                  ss_slot=Arr("ss_slot", "in", ops["ss"][order]) if "ss" in ops else None, scale_dst=Arr("scale_dst", "in", ops["sd"]) if "sd" in ops else None,
                  self=f["self"], prev=f["prev"], add=f["add"], alpha=coef[0], beta=coef[1], gamma=coef[2], out=ov,
                  ld_z=lds["z"], ld_self=lds["self"], ld_prev=lds["prev"], ld_add=lds["add"], ld_out=lds["out"])
        yield mk("gnnmp_poly_hop_ld_f32", f"{g.name}_D{D}_{mode}_{'T' if T else 'P'}_c{k % 6}_k{k}", tags, [Pl(g, T=T), job, D, STREAM], ref, no_warmup=True)
    # 2. column blocks of ONE panel [n][ld] (tests/test_recurrent_layers.py: PANELS); self in a buffer of its own with stride D, or the z
    #    block itself (cheb_conv's call); out a block of its own, or the prev / add block
    panels = [(8, 48, dict(z=0, prev=8, add=16, out=24)), (8, 45, dict(z=0, prev=8, add=16, out=24)), (6, 40, dict(z=1, prev=9, add=17, out=25)),
              (6, 42, dict(z=0, prev=6, add=12, out=18)), (260, 1100, dict(z=4, prev=268, add=532, out=796))]
    for k, (D, ld, cols) in enumerate(panels):
        for j, (g, alias) in enumerate(((ctx.hub, None), (ctx.r33, "prev"), (ctx.hub, "add"))):
            T = (k + j) % 2 == 1
            r = rng_of("poly_hop_ld_panel", g.name, D, ld, alias)
            s0, t0, n_dst, ops, order = _hop_operands(r, g, T, D, (True,) * 6)
            self_is_z = j == 2
            if self_is_z:
                ops["self_"] = ops["z"]
            coef = _hop_coef(ops)
            pan = F(r, g.n, ld)
            for nm in ("z", "prev", "add"):
                pan[:, cols[nm]:cols[nm] + D] = ops[nm]
            oc = cols[alias or "out"]
            om = np.zeros(pan.shape, bool)
            om[:, oc:oc + D] = True
            if not alias:
                pan[om] = np.nan
            P = Arr("panel", "inout", pan)
            V = lambda nm, role="in": Arr(nm, role, base=P, offset=cols[nm])      # noqa: E731

            def ref(host, a=(s0, t0, n_dst, ops, coef), pan=pan, om=om):
                full = np.zeros(pan.shape)
                full[om] = _hop_ref(*a).reshape(-1)
                return {"panel": part_E(pan, om, full)}
            job = Rec("gnnmp_poly_hop_ld_t", z=V("z"), w_slot=Arr("w_slot", "in", ops["w"][order]), ss_slot=Arr("ss_slot", "in", ops["ss"][order]),
                      scale_dst=Arr("scale_dst", "in", ops["sd"]), self=Arr("self", "in", base=P, offset=cols["z"]) if self_is_z else Arr("self", "in", ops["self_"]),
                      prev=V("prev"), add=V("add"), alpha=coef[0], beta=coef[1], gamma=coef[2], out=Arr("out", "out", base=P, offset=oc),
                      ld_z=ld, ld_self=ld if self_is_z else D, ld_prev=ld, ld_add=ld, ld_out=ld)
            tags = ({"align"} if (D, ld) in ((8, 48), (6, 42)) and alias is None else set()) | ({"ws"} if (k, j) == (0, 0) else set())
            yield mk("gnnmp_poly_hop_ld_f32", f"panel_{g.name}_D{D}_ld{ld}_{'T' if T else 'P'}_out_{alias or 'own'}{'_self_is_z' if self_is_z else ''}", tags,
                     [Pl(g, T=T), job, D, STREAM], ref, no_warmup=True)


def _nd_shapes(Ds, N0=37, align=(), extra=((1, 3), (300, 5), (300, 130))):
    """(N, D, tags) of a kernel that runs a thread an element over [N][D]"""
    for k, D in enumerate(Ds):
        yield N0, D, ({"align"} if D in align else set()) | ({"side"} if k == 0 else set())
    for N, D in extra:
        yield N, D, set()


@cases_of("gnnmp_gru_pointwise_grad_f32")
def _(ctx):
    G = _mod("gated_conv_ref")
    for k, (N, D, tags) in enumerate(_nd_shapes(G.GRU_DS, G.GRU_N, align=(3, 4, 130))):
        r = rng_of("gru_pointwise_grad", N, D)
        gx, gh, b, h, dout, base = F(r, N, 3 * D), F(r, N, 3 * D), F(r, 3 * D), F(r, N, D), F(r, N, D), F(r, N, D)
        with_b, with_base, alias = k % 2 == 0, k % 3 != 1, k % 3 == 2                     # base MAY BE dh
        dgx, dgh, dh = G.gru_grad(*[None if a is None else a.astype(f64) for a in (gx, gh, b if with_b else None, h, dout, base if with_base else None)])
        f = dict(gx=Arr("gx", "in", gx), gh=Arr("gh", "in", gh), b=Arr("b", "in", b) if with_b else None, h=Arr("h", "in", h), dout=Arr("dout", "in", dout),
                 base=Arr("base", "in", base) if with_base else None, dgx=Arr("dgx", "out", shape=(N, 3 * D)), dgh=Arr("dgh", "out", shape=(N, 3 * D)),
                 dh=Arr("dh", "out", shape=(N, D)))
        name = "dh"
        if alias:
            both = Arr("base_dh", "inout", base)
            f["base"], f["dh"], name = Arr("base", "in", base=both), Arr("dh", "out", base=both), "base_dh"
        yield mk("gnnmp_gru_pointwise_grad_f32", f"N{N}_D{D}_b{int(with_b)}_base{int(with_base)}{'_is_dh' if alias else ''}", tags,
                 [Rec("gnnmp_gru_grad_t", **f), N, D, STREAM], lambda host, v=(dgx, dgh, dh), name=name: {"dgx": v[0], "dgh": v[1], name: v[2]}, no_warmup=True)


@cases_of("gnnmp_lstm_pointwise_grad_f32")
def _(ctx):
    R = _mod("readout_ref")
    for k, (N, D, tags) in enumerate(_nd_shapes((1, 2, 3, 4, 5, 8, 33, 130), align=(3, 4, 130))):
        r = rng_of("lstm_pointwise_grad", N, D)
        gx, gh, b, c, dh, dcn = F(r, N, 4 * D), F(r, N, 4 * D), F(r, 4 * D), F(r, N, D), F(r, N, D), F(r, N, D)
        with_b, with_dcn = k % 2 == 0, k % 3 != 1
        da, dc = R.lstm_grad(*[None if a is None else a.astype(f64) for a in (gx, gh, b if with_b else None, c, dh, dcn if with_dcn else None)])
        job = Rec("gnnmp_lstm_grad_t", gx=Arr("gx", "in", gx), gh=Arr("gh", "in", gh), b=Arr("b", "in", b) if with_b else None, c=Arr("c", "in", c),
                  dh=Arr("dh", "in", dh), dcn=Arr("dcn", "in", dcn) if with_dcn else None, da=Arr("da", "out", shape=(N, 4 * D)), dc=Arr("dc", "out", shape=(N, D)))
        yield mk("gnnmp_lstm_pointwise_grad_f32", f"N{N}_D{D}_b{int(with_b)}_dcn{int(with_dcn)}", tags, [job, N, D, STREAM],
                 lambda host, v=(da, dc): {"da": v[0], "dc": v[1]}, no_warmup=True)


def _pool_shapes():
    """(D, Dg code, tags): QUERY (0), one gate weight (1), a gate per channel (2) at every width of tests/readout_ref.py"""
    R = _mod("readout_ref")
    k = 0
    for D in R.WIDTHS:
        for mode in (0, 1, 2):
            yield D, mode, ({"align"} if (D, mode) in ((8, 0), (2, 1), (130, 2), (3, 0)) else set()) | ({"side"} if k == 0 else set())
            k += 1


def _pool_operands(r, D, mode):
    R = _mod("readout_ref")
    ptr = R.ptr_of(R.SEGS_ABI)                                   # an empty segment in the middle and one at the end
    N, G = int(ptr[-1]), len(R.SEGS_ABI)
    Dg = (0, 1, D)[mode]
    x = F(r, N, D)
    q = (F(r, G, D) * (2.0 / np.sqrt(D))).astype(f32)            # logits of order one
    gate = (2.0 * F(r, N, max(Dg, 1))).astype(f32)
    return ptr, N, G, Dg, x, q if mode == 0 else None, gate if mode else None, F(r, G, D), F(r, N, D)


@cases_of("gnnmp_segment_attn_pool_f32")
def _(ctx):
    R = _mod("readout_ref")
    for D, mode, tags in _pool_shapes():
        r = rng_of("segment_attn_pool", D, mode)
        ptr, N, G, Dg, x, q, gate, _, _ = _pool_operands(r, D, mode)
        ref = lambda host, a=(x, ptr, q, gate): dict(zip(("r", "stats"), R.pool(a[0].astype(f64), a[1], *R.cast(f64, a[2], a[3]))))
        job = Rec("gnnmp_segment_attn_t", x=Arr("x", "in", x), seg_ptr=Arr("seg_ptr", "in", ptr), q=Arr("q", "in", q) if q is not None else None,
                  gate=Arr("gate", "in", gate) if gate is not None else None, r=Arr("r", "out", shape=(G, D)), stats=Arr("stats", "out", shape=(G, max(Dg, 1), 2)))
        yield mk("gnnmp_segment_attn_pool_f32", f"D{D}_Dg{Dg}_m{mode}", tags, [job, N, G, D, Dg, STREAM], ref, no_warmup=True)


@cases_of("gnnmp_segment_attn_pool_grad_f32")
def _(ctx):
    R = _mod("readout_ref")
    for k, (D, mode, tags) in enumerate(_pool_shapes()):
        r = rng_of("segment_attn_pool_grad", D, mode)
        ptr, N, G, Dg, x, q, gate, dr, base = _pool_operands(r, D, mode)
        x64, q64, g64, dr64, b64 = R.cast(f64, x, q, gate, dr, base)
        r64, st64 = R.pool(x64, ptr, q64, g64)
        how = ("base", "none", "base_is_dx", "no_dx", "only_dx")[k % 5]                      # each output is optional, base MAY BE dx
        dq, dx, dgate = R.pool_grad(dr64, x64, ptr, r64, st64, q64, g64, b64 if how in ("base", "base_is_dx") else None)
        f = dict(dr=Arr("dr", "in", dr), x=Arr("x", "in", x), seg_ptr=Arr("seg_ptr", "in", ptr), q=Arr("q", "in", q) if q is not None else None,
                 gate=Arr("gate", "in", gate) if gate is not None else None, r=Arr("r", "in", r64.astype(f32)), stats=Arr("stats", "in", st64.astype(f32)),
                 base=Arr("base", "in", base) if how == "base" else None,
                 dq=Arr("dq", "out", shape=(G, D)) if mode == 0 and how != "only_dx" else None, dx=Arr("dx", "out", shape=(N, D)) if how != "no_dx" else None,
                 dgate=Arr("dgate", "out", shape=(N, Dg)) if mode and how != "only_dx" else None)
        names = {"dq": "dq", "dx": "dx", "dgate": "dgate"}
        if how == "base_is_dx":
            both = Arr("base_dx", "inout", base)
            f["base"], f["dx"], names["dx"] = Arr("base", "in", base=both), Arr("dx", "out", base=both), "base_dx"

        def ref(host, v=dict(dq=dq, dx=dx, dgate=dgate), f=f, names=names):
            return {names[nm]: v[nm] for nm in ("dq", "dx", "dgate") if f[nm] is not None}
        yield mk("gnnmp_segment_attn_pool_grad_f32", f"D{D}_Dg{Dg}_m{mode}_{how}", tags, [Rec("gnnmp_segment_attn_grad_t", **f), N, G, D, Dg, STREAM], ref,
                 no_warmup=True)


# ---- Flux.LSTMCell at batch one (csrc/evolve.hip) --------------------------------------------------------------------------------------
def _step_operands(r, D):
    """tests/evolve_ref.py: step_inputs — Wi, Wh within ±1 / sqrt(D) (pre-activations of order one)"""
    sc = 1.0 / np.sqrt(D)
    return dict(Wi=(sc * F(r, 4 * D, D)).astype(f32), Wh=(sc * F(r, 4 * D, D)).astype(f32), x=F(r, D), h=F(r, D), c=F(r, D), b=(0.5 * F(r, 4 * D)).astype(f32),
                da=F(r, 4 * D), add_x=F(r, D), add_h=F(r, D))


EVOLVE_ALIGN = (6, 15, 64)      # 8-, 4- and 16-byte lanes: the widths at which the alignment of Wi, Wh, x, h decides


@cases_of("gnnmp_lstm_matvec_cell_f32")
def _(ctx):
    V = _mod("evolve_ref")
    k = 0
    for D in V.STEP_DS:                                            # 1056: the only width that reaches the workgroup-wide path
        for has_h, has_c, has_b, has_a, x_is_h in ((True, True, True, True, False), (False, False, False, False, False), (True, False, True, False, True)):
            r = rng_of("lstm_matvec_cell", D, has_h, has_c)
            p = _step_operands(r, D)
            if x_is_h:                                             # x and h may be the same array
                p["h"] = p["x"]
            hn, cn, a = V.step_ref(p, has_h, has_c, has_b)
            X = Arr("x", "in", p["x"])
            job = Rec("gnnmp_lstm_matvec_t", Wi=Arr("Wi", "in", p["Wi"]), Wh=Arr("Wh", "in", p["Wh"]) if has_h else None, x=X,
                      h=(Arr("h", "in", base=X) if x_is_h else Arr("h", "in", p["h"])) if has_h else None, c=Arr("c", "in", p["c"]) if has_c else None,
                      b=Arr("b", "in", p["b"]) if has_b else None, h_out=Arr("h_out", "out", shape=(D,)), c_out=Arr("c_out", "out", shape=(D,)),
                      a_out=Arr("a_out", "out", shape=(4 * D,)) if has_a else None)
            ref = lambda host, v=(hn, cn, a), has_a=has_a: {"h_out": v[0], "c_out": v[1], **({"a_out": v[2]} if has_a else {})}
            tags = ({"align"} if D in EVOLVE_ALIGN and has_h and not x_is_h else set()) | ({"side"} if k == 0 else set())
            yield mk("gnnmp_lstm_matvec_cell_f32", f"D{D}_h{int(has_h)}c{int(has_c)}b{int(has_b)}a{int(has_a)}{'_x_is_h' if x_is_h else ''}", tags,
                     [job, D, STREAM], ref, no_warmup=True)
            k += 1


@cases_of("gnnmp_lstm_matvec_grad_f32")
def _(ctx):
    from gnnmp import _lib
    V = _mod("evolve_ref")
    k = 0
    for D in V.STEP_DS:
        nws = int(_lib.load().gnnmp_lstm_matvec_grad_workspace(D))
        for how in ("both_add", "both", "x_only", "h_only_add", "sum_add", "sum"):
            r = rng_of("lstm_matvec_grad", D, how)
            p = _step_operands(r, D)
            gx, gh = V.grad_ref(p)
            want_x, want_h, add, sm = how != "h_only_add", how in ("both_add", "both", "h_only_add"), how.endswith("add"), how.startswith("sum")
            ox = (gx + gh if sm else gx) + (p["add_x"].astype(f64) if add else 0.0)
            oh = gh + (p["add_h"].astype(f64) if add else 0.0)
            job = Rec("gnnmp_lstm_matvec_grad_t", Wi=Arr("Wi", "in", p["Wi"]) if want_x else None, Wh=Arr("Wh", "in", p["Wh"]) if want_h or sm else None,
                      da=Arr("da", "in", p["da"]), add_x=Arr("add_x", "in", p["add_x"]) if add and want_x else None,
                      add_h=Arr("add_h", "in", p["add_h"]) if add and want_h else None, out_x=Arr("out_x", "out", shape=(D,)) if want_x else None,
                      out_h=Arr("out_h", "out", shape=(D,)) if want_h else None, sum=int(sm), ws=Arr("ws", "scratch", shape=(nws + 3,)), ws_floats=nws + 3)
            ref = lambda host, v=(ox, oh), w=(want_x, want_h): {**({"out_x": v[0]} if w[0] else {}), **({"out_h": v[1]} if w[1] else {})}
            tags = ({"align"} if D in EVOLVE_ALIGN and how in ("both_add", "sum") else set()) | ({"side"} if k == 0 else set())
            yield mk("gnnmp_lstm_matvec_grad_f32", f"D{D}_{how}", tags, [job, D, STREAM], ref, no_warmup=True)
            k += 1


@cases_of("gnnmp_outer_accum_f32")
def _(ctx):
    V = _mod("evolve_ref")
    # K % 4 == 0 (whole 16-byte lanes), == 2 (two floats a lane), odd; K > 1024: more than one column block to a row; R no multiple of 8
    shapes = [(3, 5, 8, {"align", "side"}), (3, 5, 6, {"align"}), (3, 5, 7, {"align"}), (1, 1, 1, ()), (4, 13, 64, ()), (3, 60, 260, ()), (2, 11, 1026, {"align"}),
              (3, 9, 1056, ()), (5, 7, 2052, ()), (3, 24, 1031, ()), (4, 4224, 6, ())]
    for k, (T, Rr, K, tags) in enumerate(shapes):
        r = rng_of("outer_accum", T, Rr, K)
        A_, B_ = F(r, T, Rr), F(r, T, K)
        dW, db = V.outer_ref(A_, B_)
        with_db = k % 2 == 0
        job = Rec("gnnmp_outer_accum_t", A=Arr("A", "in", A_), B=Arr("B", "in", B_), dW=Arr("dW", "out", shape=(Rr, K)),
                  db=Arr("db", "out", shape=(Rr,)) if with_db else None)
        yield mk("gnnmp_outer_accum_f32", f"T{T}_R{Rr}_K{K}_db{int(with_db)}", tags, [job, T, Rr, K, STREAM],
                 lambda host, v=(dW, db), with_db=with_db: {"dW": v[0], **({"db": v[1]} if with_db else {})}, no_warmup=True)


# exports neither TABLE nor PREP_TABLE covers, each with its reason (the collective; at most eight more)
EXCLUDED = {
    "gnnmp_allgather_f32": "needs an RCCL communicator (tests/test_parallel_two_ranks_gpu.py runs it between two processes)",
}
EXCLUDED_EXTRA = {
    "gnnmp_negative_sample": "random draws with a host-side trial loop: no deterministic reference for the written prefix (tests/test_linkpred.py: properties)",
    "gnnmp_sample_neighbors": "random draws: parity is distributional (tests/test_graphprep.py); the written prefix has no exact reference",
    "gnnmp_debug_random_walk_pe_f32": "GNNMP_INTERNAL test hook: gnnmp_random_walk_pe_f32 (which IS in the table) with another LDS budget; the header documents "
                                      "no stream behaviour of its own for it, so it can be neither recorded nor quoted as exempt (tests/test_rwpe.py drives it)",
}


# ---- MEGNetConv (csrc/megnet.hip) --------------------------------------------------------------------------------------------------------
ACT_NAMES = ("identity", "relu", "softplus", "tanh", "swish")          # gnnmp_act, IDENTITY .. SWISH
EDGE_DS = (1, 2, 3, 6, 7, 64, 100, 260)                                # tests/megnet_conv_ref.py: WIDTHS — 4- / 8- / 16-byte lanes, tails, a second feature tile
EDGE_SHAPES = dict(Ds=EDGE_DS, small=(3, 64), align=(3, 6, 64), ws=(6,), rows300=(1, 260))


@cases_of("gnnmp_megnet_edge_f32")
def _(ctx):
    M = _mod("megnet_conv_ref")
    for k, (g, D, tags) in enumerate(ctx.graph_shapes(**EDGE_SHAPES)):
        act, with_F, with_z = k % 5, k % 2 == 0, k % 3 != 1
        r = rng_of("megnet_edge", g.name, D)
        P, Q, Fe = F(r, g.n, D), F(r, g.n, D), F(r, g.E, D)
        a0, z0 = M.edge(g.s - 1, g.t - 1, P.astype(f64), Q.astype(f64), Fe.astype(f64) if with_F else None, ACT_NAMES[act])
        job = Rec("gnnmp_megnet_edge_t", P=Arr("P", "in", P), Q=Arr("Q", "in", Q), F=Arr("F", "in", Fe) if with_F else None, a0=Arr("a0", "out", shape=(g.E, D)),
                  z0=Arr("z0", "out", shape=(g.E, D)) if with_z else None, act=act)
        yield mk("gnnmp_megnet_edge_f32", f"{g.name}_D{D}_act{act}_F{int(with_F)}_z{int(with_z)}", tags, [Pl(g), job, D, STREAM],
                 lambda host, v=(a0, z0), with_z=with_z: {"a0": v[0], **({"z0": v[1]} if with_z else {})}, no_warmup=True)


@cases_of("gnnmp_megnet_edge_grad_f32")
def _(ctx):
    M = _mod("megnet_conv_ref")
    for k, (g, D, tags) in enumerate(ctx.graph_shapes(**EDGE_SHAPES)):
        act = k % 5
        want = (("dz0", "dP", "dQ"), ("dP", "dQ"), ("dz0",))[k % 3]
        r = rng_of("megnet_edge_grad", g.name, D)
        da0, z = F(r, g.E, D), F(r, g.E, D)
        dz, dP, dQ = M.edge_grad(g.s - 1, g.t - 1, g.n, da0.astype(f64), z.astype(f64), ACT_NAMES[act])
        job = Rec("gnnmp_megnet_edge_grad_t", da0=Arr("da0", "in", da0), z=Arr("z", "in", z) if act or k % 2 else None,
                  dz0=Arr("dz0", "out", shape=(g.E, D)) if "dz0" in want else None, dP=Arr("dP", "out", shape=(g.n, D)) if "dP" in want else None,
                  dQ=Arr("dQ", "out", shape=(g.n, D)) if "dQ" in want else None, act=act)
        yield mk("gnnmp_megnet_edge_grad_f32", f"{g.name}_D{D}_act{act}_{'_'.join(want)}", tags, [Pl(g), Pl(g, T=True), job, D, STREAM],
                 lambda host, v=dict(dz0=dz, dP=dP, dQ=dQ), want=want: {nm: v[nm] for nm in want}, no_warmup=True)


@cases_of("gnnmp_aggregate_grad_f32")
def _(ctx):
    M = _mod("megnet_conv_ref")
    for k, (g, D, tags) in enumerate(ctx.graph_shapes(**EDGE_SHAPES)):
        aggr, with_acc = k % 4, k % 3 != 0
        name = M.AGGRS[aggr]
        r = rng_of("aggregate_grad", g.name, D)
        dy, m, acc = F(r, g.n_dst, D), F(r, g.E, D), F(r, g.E, D)
        if k % 2 == 0:
            m = (np.round(m * 4) / 4).astype(f32)                      # ties inside a row: EVERY tying copy gets the whole Δ
        y = M.aggregate(g.t - 1, g.n_dst, m, name)                      # float32 max / min: exact
        dm = M.aggregate_grad(g.t - 1, g.n_dst, dy.astype(f64), m.astype(f64), y.astype(f64), name, acc.astype(f64) if with_acc else None)
        need = aggr in (MAX, MIN)
        job = Rec("gnnmp_aggregate_grad_t", dy=Arr("dy", "in", dy), m=Arr("m", "in", m) if need or k % 2 else None, y=Arr("y", "in", y) if need or k % 2 else None,
                  acc=Arr("acc", "in", acc) if with_acc else None, dm=Arr("dm", "out", shape=(g.E, D)))
        yield mk("gnnmp_aggregate_grad_f32", f"{g.name}_D{D}_a{aggr}_acc{int(with_acc)}", tags, [Pl(g), job, aggr, D, STREAM], lambda host, dm=dm: {"dm": dm},
                 no_warmup=True)


# ---- EGNNConv (csrc/egnn.hip) ------------------------------------------------------------------------------------------------------------
DXS = (1, 2, 3, 4, 7, 16)                                               # tests/egnn_conv_ref.py: DXS (a node's coordinates stay in registers: Dx <= 16)
COORD_SHAPES = dict(Ds=DXS, small=(3, 16), align=(3, 4), ws=(4,), rows300=(1, 16))


def _coords(r, n, Dx):
    """coordinates of order one with one pair of coincident points (q = 0 between them; the graphs' self loops give q = 0 too)"""
    x = (2.0 * F(r, n, Dx)).astype(f32)
    if n > 2:
        x[n // 2] = x[0]
    return x


@cases_of("gnnmp_egnn_edge_f32")
def _(ctx):
    G = _mod("egnn_conv_ref")
    shapes = [(33, hid, ({"align"} if hid in (3, 6, 8) else set()) | ({"side"} if j == 0 else set())) for j, hid in enumerate(G.HIDS)]
    shapes += [(1, 3, set()), (31, 64, set()), (300, 1, set()), (300, 260, set())]
    for k, (K, hid, tags) in enumerate(shapes):
        ib, base = IDX[k % 4]
        Dx, act, with_F, with_z = DXS[k % 6], k % 5, k % 2 == 0, k % 3 != 1
        r = rng_of("egnn_edge", K, hid)
        n = 40
        s1, t1 = r.integers(1, n + 1, K), r.integers(1, n + 1, K)
        x, P, Q, Fe, c = _coords(r, n, Dx), F(r, n, hid), F(r, n, hid), F(r, K, hid), (G.C_SCALE * F(r, hid)).astype(f32)
        q, z0, a0 = G.edge_ref(s1 - 1, t1 - 1, x, P, Q, Fe if with_F else None, c, ACT_NAMES[act])
        job = Rec("gnnmp_egnn_edge_t", s=Arr("s", "in", IX(s1, ib, base)), t=Arr("t", "in", IX(t1, ib, base)), idx_bytes=ib, index_base=base, x=Arr("x", "in", x),
                  P=Arr("P", "in", P), Q=Arr("Q", "in", Q), F=Arr("F", "in", Fe) if with_F else None, c=Arr("c", "in", c), q=Arr("q", "out", shape=(K,)),
                  a0=Arr("a0", "out", shape=(K, hid)), z0=Arr("z0", "out", shape=(K, hid)) if with_z else None, act=act)
        yield mk("gnnmp_egnn_edge_f32", f"K{K}_hid{hid}_Dx{Dx}_act{act}_F{int(with_F)}_z{int(with_z)}_i{ib}b{base}", tags, [job, K, hid, Dx, STREAM],
                 lambda host, v=(q, a0, z0), with_z=with_z: {"q": v[0], "a0": v[1], **({"z0": v[2]} if with_z else {})}, no_warmup=True)


@cases_of("gnnmp_egnn_coord_f32")
def _(ctx):
    G = _mod("egnn_conv_ref")
    for g, Dx, tags in ctx.graph_shapes(**COORD_SHAPES):
        r = rng_of("egnn_coord", g.name, Dx)
        x, mx = _coords(r, g.n, Dx), F(r, g.E)
        xo = G.coord_ref(g.s - 1, g.t - 1, g.n, x, mx)
        job = Rec("gnnmp_egnn_coord_t", x=Arr("x", "in", x), mx=Arr("mx", "in", mx), xo=Arr("xo", "out", shape=(g.n, Dx)))
        yield mk("gnnmp_egnn_coord_f32", f"{g.name}_Dx{Dx}", tags, [Pl(g), job, Dx, STREAM], lambda host, xo=xo: {"xo": xo}, no_warmup=True)


@cases_of("gnnmp_egnn_coord_grad_f32")
def _(ctx):
    G = _mod("egnn_conv_ref")
    for k, (g, Dx, tags) in enumerate(ctx.graph_shapes(**COORD_SHAPES)):
        want = (("dmx", "dx"), ("dx",), ("dmx",))[k % 3]
        r = rng_of("egnn_coord_grad", g.name, Dx)
        x, dxo, mx, dq = _coords(r, g.n, Dx), F(r, g.n, Dx), F(r, g.E), F(r, g.E)
        with np.errstate(divide="ignore", invalid="ignore"):
            dmx, dx = G.coord_grad_ref(g.s - 1, g.t - 1, g.n, x, dxo, mx, dq)
        job = Rec("gnnmp_egnn_coord_grad_t", x=Arr("x", "in", x), dxo=Arr("dxo", "in", dxo), mx=Arr("mx", "in", mx) if "dx" in want or k % 2 else None,
                  dq=Arr("dq", "in", dq) if "dx" in want or k % 2 else None, dmx=Arr("dmx", "out", shape=(g.E,)) if "dmx" in want else None,
                  dx=Arr("dx", "out", shape=(g.n, Dx)) if "dx" in want else None)
        yield mk("gnnmp_egnn_coord_grad_f32", f"{g.name}_Dx{Dx}_{'_'.join(want)}", tags, [Pl(g), Pl(g, T=True), job, Dx, STREAM],
                 lambda host, v=dict(dmx=dmx, dx=dx), want=want: {nm: v[nm] for nm in want}, no_warmup=True)


@cases_of("gnnmp_act_grad_z_f32")
def _(ctx):
    G = _mod("egnn_conv_ref")
    k = 0
    for n in G.ACT_NS + (4100,):                                       # 4099: a tail of the 16-byte lanes; 4100: none
        for act in range(5):
            r = rng_of("act_grad_z", n, act)
            dy, z = F(r, n), (3.0 * F(r, n)).astype(f32)
            dz = G.act_grad_z_ref(dy, z, ACT_NAMES[act])
            job = Rec("gnnmp_act_grad_z_t", dy=Arr("dy", "in", dy), z=Arr("z", "in", z) if act or n % 2 else None, dz=Arr("dz", "out", shape=(n,)), act=act)
            tags = ({"align"} if n in (5, 4100) and act in (1, 4) else set()) | ({"side"} if k == 0 else set())
            yield mk("gnnmp_act_grad_z_f32", f"n{n}_act{act}", tags, [job, n, STREAM], lambda host, dz=dz: {"dz": dz}, no_warmup=True)
            k += 1


# ---- GMMConv (csrc/gmm.hip) ----------------------------------------------------------------------------------------------------------------
GMM_SHAPES = dict(Ds=(1, 2, 3, 4, 5, 8, 33, 64, 130), small=(3, 8), align=(3, 2, 8), ws=(4,), rows300=(1, 130))      # tests/gmm_conv_ref.py: KERNEL_CS


@cases_of("gnnmp_gmm_conv_f32")
def _(ctx):
    G = _mod("gmm_conv_ref")
    for k, (g, C, tags) in enumerate(ctx.graph_shapes(**GMM_SHAPES)):
        K = G.KERNEL_KS[k % 6] if C <= 33 else 3
        act, with_b, with_z = k % 5, k % 2 == 0, k % 3 != 1
        r = rng_of("gmm_conv", g.name, C)
        w, xk, bias = (0.25 + 0.75 * r.random((g.E, K))).astype(f32), F(r, g.n, K * C), F(r, C)
        z = G.rows(g.s - 1, g.t - 1, g.n, w.astype(f64), xk.astype(f64), bias.astype(f64) if with_b else None, K, C)
        y = G.act(z, ACT_NAMES[act])
        job = Rec("gnnmp_gmm_conv_t", w=Arr("w", "in", w), xk=Arr("xk", "in", xk), bias=Arr("bias", "in", bias) if with_b else None, y=Arr("y", "out", shape=(g.n, C)),
                  z=Arr("z", "out", shape=(g.n, C)) if with_z else None, act=act)
        yield mk("gnnmp_gmm_conv_f32", f"{g.name}_C{C}_K{K}_act{act}_b{int(with_b)}_z{int(with_z)}", tags, [Pl(g), job, K, C, STREAM],
                 lambda host, v=(y, z), with_z=with_z: {"y": v[0], **({"z": v[1]} if with_z else {})}, no_warmup=True)


@cases_of("gnnmp_gmm_conv_grad_f32")
def _(ctx):
    G = _mod("gmm_conv_ref")
    for k, (g, C, tags) in enumerate(ctx.graph_shapes(**GMM_SHAPES)):
        K = G.KERNEL_KS[k % 6] if C <= 33 else 3
        want = (("dxk", "dw"), ("dxk",), ("dw",))[k % 3]
        r = rng_of("gmm_conv_grad", g.name, C)
        w, xk, dz = (0.25 + 0.75 * r.random((g.E, K))).astype(f32), F(r, g.n, K * C), F(r, g.n, C)
        dxk, dw = G.rows_grad(g.s - 1, g.t - 1, g.n, w.astype(f64), xk.astype(f64), dz.astype(f64), K, C)
        job = Rec("gnnmp_gmm_conv_grad_t", w=Arr("w", "in", w) if "dxk" in want or k % 2 else None, xk=Arr("xk", "in", xk) if "dw" in want or k % 2 else None,
                  dz=Arr("dz", "in", dz), dxk=Arr("dxk", "out", shape=(g.n, K * C)) if "dxk" in want else None, dw=Arr("dw", "out", shape=(g.E, K)) if "dw" in want else None)
        yield mk("gnnmp_gmm_conv_grad_f32", f"{g.name}_C{C}_K{K}_{'_'.join(want)}", tags, [Pl(g), Pl(g, T=True), job, K, C, STREAM],
                 lambda host, v=dict(dxk=dxk, dw=dw), want=want: {nm: v[nm] for nm in want}, no_warmup=True)


# ---- EdgeConv, CGConv, NNConv: the training kernels (csrc/edge_conv.hip, cg_grad.hip, nn_grad.hip) -----------------------------------------
CONV_SHAPES = dict(Ds=(1, 3, 6, 8, 64, 260), small=(3, 8), align=(3, 6, 8), ws=(6,), rows300=(1, 260))      # tests/cg_conv_ref.py: KERNEL_CS


@cases_of("gnnmp_edge_conv_f32")
def _(ctx):
    V = _mod("edge_conv_ref")
    for k, (g, C, tags) in enumerate(ctx.graph_shapes(**CONV_SHAPES)):
        aggr, act = k % 4, (k // 2) % 2
        r = rng_of("edge_conv", g.name, C)
        P = F(r, g.n, 2 * C)
        # the header: every row is folded sequentially in edge order, each operation rounded on its own — the float32 restatement has the bits
        y = V.fused(g.s - 1, g.t - 1, g.n, P, C, V.AGGRS[aggr], V.ACTS[act])[0]
        job = Rec("gnnmp_edge_conv_t", p=Arr("p", "in", P), y=Arr("y", "out", shape=(g.n, C)), aggr=aggr, act=act)
        yield mk("gnnmp_edge_conv_f32", f"{g.name}_C{C}_a{aggr}_act{act}", tags, [Pl(g), job, C, STREAM], lambda host, y=y: {"y": E(y, "exact")}, no_warmup=True)


@cases_of("gnnmp_edge_conv_grad_f32")
def _(ctx):
    V = _mod("edge_conv_ref")
    for k, (g, C, tags) in enumerate(ctx.graph_shapes(**CONV_SHAPES)):
        aggr, act = k % 4, (k // 2) % 2
        r = rng_of("edge_conv_grad", g.name, C)
        P, dy = F(r, g.n, 2 * C), F(r, g.n, C)
        if k % 3 == 0:
            P = (np.round(P * 4) / 4).astype(f32)                       # ties under max / min, pre-activations at 0 under relu
        y = V.fused(g.s - 1, g.t - 1, g.n, P, C, V.AGGRS[aggr], V.ACTS[act])[0]
        dp = V.grad_p(g.s - 1, g.t - 1, g.n, P, C, y, dy, V.AGGRS[aggr], V.ACTS[act])          # float32: "the bits of the kernels"
        job = Rec("gnnmp_edge_conv_grad_t", p=Arr("p", "in", P), y=Arr("y", "in", y), dy=Arr("dy", "in", dy), dp=Arr("dp", "out", shape=(g.n, 2 * C)), aggr=aggr, act=act)
        yield mk("gnnmp_edge_conv_grad_f32", f"{g.name}_C{C}_a{aggr}_act{act}", tags, [Pl(g), Pl(g, T=True), job, C, STREAM],
                 lambda host, dp=dp: {"dp": E(dp, "exact")}, no_warmup=True)


@cases_of("gnnmp_cg_conv_grad_f32")
def _(ctx):
    V = _mod("cg_conv_ref")
    for k, (g, C, tags) in enumerate(ctx.graph_shapes(**CONV_SHAPES)):
        act, with_e = k % 4, k % 2 == 0
        want_e = with_e and k % 4 == 0
        for salt in range(16):                                          # relu: no pre-activation of dense_s within float32 rounding of its kink
            r = rng_of("cg_conv_grad", g.name, C, salt)
            fi, fj, fe, dy = F(r, g.n, 2 * C), F(r, g.n, 2 * C), F(r, g.E, 2 * C), F(r, g.n, C)
            sp = V.pre(g.s - 1, g.t - 1, fi, fj, fe if with_e else None, C)[1]
            if act != 1 or not sp.size or np.abs(sp).min() > 1e-5:
                break
        di, dj, de = V.rows_grad(g.s - 1, g.t - 1, g.n, fi.astype(f64), fj.astype(f64), fe.astype(f64) if with_e else None, dy.astype(f64), C, V.ACTS[act])
        job = Rec("gnnmp_cg_conv_grad_t", fs_i=Arr("fs_i", "in", fi), fs_j=Arr("fs_j", "in", fj), fs_e=Arr("fs_e", "in", fe) if with_e else None, dy=Arr("dy", "in", dy),
                  dfs_i=Arr("dfs_i", "out", shape=(g.n, 2 * C)), dfs_j=Arr("dfs_j", "out", shape=(g.n, 2 * C)),
                  dfs_e=Arr("dfs_e", "out", shape=(g.E, 2 * C)) if want_e else None, act=act)
        yield mk("gnnmp_cg_conv_grad_f32", f"{g.name}_C{C}_act{act}_e{int(with_e)}{int(want_e)}", tags, [Pl(g), Pl(g, T=True), job, C, STREAM],
                 lambda host, v=(di, dj, de), want_e=want_e: {"dfs_i": v[0], "dfs_j": v[1], **({"dfs_e": v[2]} if want_e else {})}, no_warmup=True)


@cases_of("gnnmp_nn_conv_grad_f32")
def _(ctx):
    V = _mod("nn_conv_ref")
    shapes = [(ctx.hub, Din, Dout, ({"align"} if (Din, Dout) in ((3, 5), (8, 8), (33, 20)) else set()) | ({"side", "ws"} if j == 0 else set()))
              for j, (Din, Dout) in enumerate(V.KERNEL_SHAPES)]                   # every lane geometry; two feature tiles at (3, 130), (2, 260)
    shapes += [(ctx.e0, 3, 4, ()), (ctx.one, 4, 3, ()), (ctx.r31, 2, 6, ()), (ctx.r33, 5, 3, ()), (ctx.r300, 4, 8, ()), (ctx.r300, 3, 1, ()), (ctx.r300, 2, 70, ())]
    for k, (g, Din, Dout, tags) in enumerate(shapes):
        want = (("dx", "dwe"), ("dx",), ("dwe",))[k % 3]
        r = rng_of("nn_conv_grad", g.name, Din, Dout)
        x, we, dm = F(r, g.n, Din), F(r, g.E, Dout * Din), F(r, g.n, Dout)
        dx, dwe = V.rows_grad64(g.s - 1, g.t - 1, g.n, x, we, dm, Din, Dout)
        job = Rec("gnnmp_nn_conv_grad_t", x=Arr("x", "in", x), we=Arr("we", "in", we) if "dx" in want or k % 2 else None, dm=Arr("dm", "in", dm),
                  dx=Arr("dx", "out", shape=(g.n, Din)) if "dx" in want else None, dwe=Arr("dwe", "out", shape=(g.E, Dout * Din)) if "dwe" in want else None)
        yield mk("gnnmp_nn_conv_grad_f32", f"{g.name}_{Din}x{Dout}_{'_'.join(want)}", tags, [Pl(g, T=True), job, Din, Dout, STREAM],
                 lambda host, v=dict(dx=dx, dwe=dwe), want=want: {nm: v[nm] for nm in want}, no_warmup=True)


# ---- attention with a per-edge feature row (csrc/attn_edge.hip) ------------------------------------------------------------------------------
EDGE_WIDE = WIDE + ("F", "dF")      # "F and dF count among the [.][H*C] arrays whose alignment selects v"


def _attn_edge_operands(r, g, H, C):
    D = H * C
    return dict(Q=F(r, g.n, D), K=F(r, g.n, D), V=F(r, g.n, D), F=F(r, g.E, D), a=F(r, H, C), bias=F(r, D), dout=F(r, g.n, D))


def _attn_edge_core(g, mode, i, H, C, sepQ, sepV, slope, scale):
    V = _mod("attn_edge_ref")
    sh = lambda k: i[k].astype(f64).reshape(-1, H, C)      # noqa: E731
    Q, K = sh("Q") if sepQ else sh("K"), sh("K")
    args = ("gatv2" if mode == 1 else "dot", g.s - 1, g.t - 1, g.n, Q, K, sh("V") if sepV else K, sh("F"), i["a"].astype(f64), slope, scale)
    o, c = V.core(*args)
    return o, c, args


def _edge_align(H, C, base=None):
    d = dict(base or {})
    if H * C > 64:
        d.update({n: EUNSUPPORTED for n in EDGE_WIDE})
    return d


@cases_of("gnnmp_attn_conv_edge_f32")
def _(ctx):
    for k, (g, H, C, tags) in enumerate(att_shapes(ctx, False)):
        mode = 1 + k % 2                                                # GNNMP_ATTN_GATV2 | GNNMP_ATTN_DOT
        sepQ, sepV, with_b, act, with_stats = k % 3 != 2, mode == 2 and k % 4 < 2, k % 2 == 0 or k % 3 == 0, (k // 2) % 2, k % 3 != 1
        slope, scale = 0.2, float(np.float32(np.sqrt(np.float32(C))))
        r = rng_of("attn_conv_edge", g.name, H, C)
        i = _attn_edge_operands(r, g, H, C)
        o, c, _ = _attn_edge_core(g, mode, i, H, C, sepQ, sepV, slope, scale)
        out = o.reshape(g.n, H * C) + (i["bias"].astype(f64) if with_b else 0.0)
        out = np.maximum(out, 0.0) if act else out
        stats = np.stack([c["m"], c["den"]], axis=-1)
        job = Rec("gnnmp_attn_edge_t", Q=Arr("Q", "in", i["Q"]) if sepQ else None, K=Arr("K", "in", i["K"]), V=Arr("V", "in", i["V"]) if sepV else None,
                  F=Arr("F", "in", i["F"]), a=Arr("a", "in", i["a"]) if mode == 1 or k % 3 == 0 else None, bias=Arr("bias", "in", i["bias"]) if with_b else None,
                  out=Arr("out", "out", shape=(g.n, H * C)), stats=Arr("stats", "out", shape=(g.n, H, 2)) if with_stats else None,
                  negative_slope=slope, scale=scale, act=act)
        yield mk("gnnmp_attn_conv_edge_f32", f"{g.name}_m{mode}_H{H}_C{C}_q{int(sepQ)}v{int(sepV)}", tags, [Pl(g), mode, job, H, C, STREAM],
                 lambda host, v=(out, stats), with_stats=with_stats: {"out": v[0], **({"stats": v[1]} if with_stats else {})},
                 align_status=_edge_align(H, C), no_warmup=True)


@cases_of("gnnmp_attn_conv_edge_grad_f32")
def _(ctx):
    V = _mod("attn_edge_ref")
    for k, (g, H, C, tags) in enumerate(att_shapes(ctx, False)):
        mode = 1 + k % 2
        sepQ, sepV, with_da = k % 3 != 2, mode == 2 and k % 4 < 2, k % 3 != 1
        slope, scale = 0.2, float(np.float32(np.sqrt(np.float32(C))))
        D = H * C
        r = rng_of("attn_conv_edge_grad", g.name, H, C)
        i = _attn_edge_operands(r, g, H, C)
        o, c, args = _attn_edge_core(g, mode, i, H, C, sepQ, sepV, slope, scale)
        gr = V.core_grad(*args, c, i["dout"].astype(f64).reshape(-1, H, C))
        stats = np.stack([c["m"], c["den"]], axis=-1).astype(f32)
        want = {nm: gr[nm].reshape(-1, D) for nm in ("dQ", "dK", "dF")}
        if mode == 2:
            want["dV"] = gr["dV"].reshape(-1, D)
        else:
            want["dA"] = gr["dA"].reshape(-1, D)
            if with_da:
                want["da"] = gr["da"]
        # dl = α (g − D) is a DIFFERENCE of float64 terms that cancels to (almost) zero where a row's edges carry equal values — the
        # one-node graph's two self loops: float32 rounding lives on the scale of the terms α g and α D times the factor they meet, so
        # that is the floor of "the reference's scale", per destination row (dQ, dA), source row (dK), edge (dF) or over all (da) —
        # the floors of the e-less pullbacks above (attn_ref: gscale).  dV = Σ α Δ has no difference in it
        al = c["al"]
        gg = (i["dout"].astype(f64).reshape(-1, H, C)[g.t - 1] * c["val"]).sum(-1)
        big = max([1.0] + [float(np.abs(i[nm]).max()) for nm in ("Q", "K", "V", "F", "a") if i[nm].size])
        term = big * (np.abs(al * gg) + np.abs(al * gr["D"][g.t - 1])).max(-1) if g.E else np.zeros(0)
        row_t, row_s = np.zeros(g.n), np.zeros(g.n)
        np.maximum.at(row_t, g.t - 1, term)
        np.maximum.at(row_s, g.s - 1, term)
        floors = dict(dQ=row_t, dA=row_t, dK=row_s, dF=term if g.E else 0.0, da=float(term.max()) if g.E else 0.0, dV=0.0)
        ref = lambda host, want=want, floors=floors: {nm: E(v, scale=floors[nm]) for nm, v in want.items()}
        job = Rec("gnnmp_attn_edge_grad_t", Q=Arr("Q", "in", i["Q"]) if sepQ else None, K=Arr("K", "in", i["K"]), V=Arr("V", "in", i["V"]) if sepV else None,
                  F=Arr("F", "in", i["F"]), a=Arr("a", "in", i["a"]) if mode == 1 else None, stats=Arr("stats", "in", stats), dout=Arr("dout", "in", i["dout"]),
                  line=Arr("line", "scratch", shape=(g.n, H, 4)), dQ=Arr("dQ", "out", shape=(g.n, D)), dK=Arr("dK", "out", shape=(g.n, D)),
                  dV=Arr("dV", "out", shape=(g.n, D)) if mode == 2 else None, dF=Arr("dF", "out", shape=(g.E, D)),
                  dA=Arr("dA", "out", shape=(g.n, D)) if mode == 1 else None, da=Arr("da", "out", shape=(H, C)) if mode == 1 and with_da else None,
                  negative_slope=slope, scale=scale)
        yield mk("gnnmp_attn_conv_edge_grad_f32", f"{g.name}_m{mode}_H{H}_C{C}_q{int(sepQ)}v{int(sepV)}", tags, [Pl(g), Pl(g, T=True), mode, job, H, C, STREAM],
                 ref, align_status=_edge_align(H, C, LINE_ALIGN), no_warmup=True)


# ---- heterographs: tables of relation records (csrc/hetero.hip, hetero_backward.hip) ------------------------------------------------------------
HET_SHAPES = dict(Ds=(1, 3, 6, 8, 129, 260), small=(3, 8), align=(3, 6, 8), ws=(8,), rows300=(1, 260))
AGGR_NAMES = ("+", "mean", "max", "min")


def _bipartite(ctx, name, n_src, n_dst, E_, seed):
    """a relation between two node types, made once per Ctx (plans are keyed on the Graph object)"""
    if name not in ctx.cache:
        ctx.cache[name] = random_graph(name, n_src, E_, seed, n_dst=n_dst)
    return ctx.cache[name]


@cases_of("gnnmp_hetero_propagate_f32")
def _(ctx):
    H = _mod("hetero_ref")
    for k, (g, D, tags) in enumerate(ctx.graph_shapes(**HET_SHAPES)):
        r = rng_of("hetero_propagate", g.name, D)
        n, m = g.n, 17
        gb = _bipartite(ctx, f"het_b_{g.name}", m, n, 3 * n, 11)          # type B (17 nodes) -> type A (the graph's nodes)
        gc = _bipartite(ctx, f"het_c_{g.name}", n, m, 2 * n + 5, 12)      # type A -> type B
        xa, xb, root, w = F(r, n, D), F(r, m, D), F(r, n, D), F(r, g.E)
        a1, a2, a3 = AGGR_NAMES[k % 4], AGGR_NAMES[(k + 1) % 4], AGGR_NAMES[(k + 2) % 4]
        comb0, comb1 = (SUM, MAX, MIN)[k % 3], (SUM, MAX, MIN)[(k + 1) % 3]
        cname = {SUM: "+", MAX: "max", MIN: "min"}
        # table order: the root term (an identity relation), the weighted relation inside type A, the relation from type B
        out0 = H.hetero_ref([(g.s - 1, g.t - 1, xa, w, a1), (gb.s - 1, gb.t - 1, xb, None, a2)], n, cname[comb0], root=root)
        out1 = H.hetero_ref([(gc.s - 1, gc.t - 1, xa, None, a3)], m, cname[comb1])
        XA = Arr("x_a", "in", xa, field="x")
        dsts = [Rec("gnnmp_hetero_dst_t", out=Arr("out_a", "out", shape=(n, D), field="out"), n_dst=n, combine=comb0, n_rel=3, rels=[
                    Rec("gnnmp_hetero_rel_t", plan=None, x=Arr("root", "in", root, field="x"), w=None, aggr=SUM),
                    Rec("gnnmp_hetero_rel_t", plan=Pl(g), x=XA, w=Arr("w", "in", w), aggr=k % 4),
                    Rec("gnnmp_hetero_rel_t", plan=Pl(gb), x=Arr("x_b", "in", xb, field="x"), w=None, aggr=(k + 1) % 4)]),
                Rec("gnnmp_hetero_dst_t", out=Arr("out_b", "out", shape=(m, D), field="out"), n_dst=m, combine=comb1, n_rel=1, rels=[
                    Rec("gnnmp_hetero_rel_t", plan=Pl(gc), x=Arr("x_a2", "in", base=XA, field="x"), w=None, aggr=(k + 2) % 4)])]
        # "bit-identical to the sequential loop": the float32 restatement of tests/hetero_ref.py has the bits, on every row
        yield mk("gnnmp_hetero_propagate_f32", f"{g.name}_D{D}_a{k % 4}_c{comb0}{comb1}", tags, [dsts, 2, D, STREAM],
                 lambda host, v=(out0, out1): {"out_a": E(v[0], "exact"), "out_b": E(v[1], "exact")}, no_warmup=True)


@cases_of("gnnmp_hetero_propagate_grad_f32")
def _(ctx):
    H, HG = _mod("hetero_ref"), _mod("hetero_grad_ref")
    for k, (g, D, tags) in enumerate(ctx.graph_shapes(**HET_SHAPES)):
        r = rng_of("hetero_propagate_grad", g.name, D)
        n, m = g.n, 17
        gc = _bipartite(ctx, f"het_c_{g.name}", n, m, 2 * n + 5, 12)      # type A -> type B
        gb = _bipartite(ctx, f"het_b_{g.name}", m, n, 3 * n, 11)          # type B -> type A
        xa, xb = F(r, n, D), F(r, m, D)
        if k % 2 == 0:
            xa = (np.round(xa * 4) / 4).astype(f32)                       # ties: every tie receives the gradient
        dy_a, dy_b, dy_id, w, sd = F(r, n, D), F(r, m, D), F(r, n, D), F(r, g.E), (0.5 + r.random(n)).astype(f32)
        mx = "max" if k % 2 == 0 else "min"
        y_b = H.propagate_ref(gc.s - 1, gc.t - 1, m, xa, None, mx)        # the forward aggregate of A -> B under max / min, float32
        term = F(r, n, D)
        out_fold = np.maximum(term, xa) if k % 2 == 0 else np.minimum(term, xa)      # the fold's result: `term` ties with it where it won
        use_w, use_sd = k % 3 != 1, k % 3 != 2
        c = [HG.linear_ref(g.s - 1, g.t - 1, n, dy_a, w if use_w else None, sd if use_sd else None),      # + / mean inside type A
             HG.winners_ref(gc.s - 1, gc.t - 1, n, xa, y_b, dy_b),                                            # max / min towards type B
             dy_id.copy(),                                                                                    # a root term
             HG.masked_ref(term, out_fold, dy_id)]                                                            # one term of a max / min fold
        dxa = HG.sum_ref(c)
        dxb = HG.sum_ref([HG.linear_ref(gb.s - 1, gb.t - 1, m, dy_a, None, None)])
        DYA, DYI = Arr("dy_a", "in", dy_a, field="dy"), Arr("dy_id", "in", dy_id, field="dy")
        R_ = lambda **f: Rec("gnnmp_hetero_rel_grad_t", **f)      # noqa: E731
        srcs = [Rec("gnnmp_hetero_src_t", dx=Arr("dx_a", "out", shape=(n, D), field="dx"), x=Arr("x_a", "in", xa, field="x"), n_src=n, n_rel=4, rels=[
                    R_(plan_t=Pl(g, T=True), dy=DYA, w=Arr("w", "in", w) if use_w else None, sd=Arr("sd", "in", sd) if use_sd else None, y=None, out=None),
                    R_(plan_t=Pl(gc, T=True), dy=Arr("dy_b", "in", dy_b, field="dy"), w=None, sd=None, y=Arr("y_b", "in", y_b, field="y"), out=None),
                    R_(plan_t=None, dy=DYI, w=None, sd=None, y=None, out=None),
                    R_(plan_t=None, dy=Arr("dy_id2", "in", base=DYI, field="dy"), w=None, sd=None, y=Arr("term", "in", term, field="y"),
                       out=Arr("out_fold", "in", out_fold, field="out"))]),
                Rec("gnnmp_hetero_src_t", dx=Arr("dx_b", "out", shape=(m, D), field="dx"), x=None if k % 2 else Arr("x_b", "in", xb, field="x"), n_src=m, n_rel=1,
                    rels=[R_(plan_t=Pl(gb, T=True), dy=Arr("dy_a2", "in", base=DYA, field="dy"), w=None, sd=None, y=None, out=None)])]
        yield mk("gnnmp_hetero_propagate_grad_f32", f"{g.name}_D{D}_{mx}_w{int(use_w)}sd{int(use_sd)}", tags, [srcs, 2, D, STREAM],
                 lambda host, v=(dxa, dxb): {"dx_a": E(v[0], "exact"), "dx_b": E(v[1], "exact")}, no_warmup=True)


# ---- graph prep through records: coalescing, compaction, random-walk encodings (they synchronise: SYNCHRONISES below) ---------------------------
@cases_of("gnnmp_coalesce_edges")
def _(ctx):
    TR = _mod("transforms_ref")
    k = 0
    for n, E_ in PREP[:4]:
        for mode in (0, 1, 2):                                          # DIRECTED, MIRRORED, UNDIRECTED
            ib, base = IDX[k % 4]
            r = rng_of("coalesce", n, E_, mode)
            s1, t1 = r.integers(1, n + 1, E_), r.integers(1, n + 1, E_)
            s1[E_ // 2:] = s1[:E_ - E_ // 2]                           # parallel edges
            t1[E_ // 2:] = t1[:E_ - E_ // 2]
            c = (TR.remove_multi_edges, TR.to_bidirected, TR.to_unidirected)[mode](s1, t1, n)
            Ev = 2 * E_ if mode == 1 else E_                            # the virtual list of to_bidirected is never materialised
            tot = len(c.s)
            colptr = np.concatenate([[0], np.cumsum(c.seg_len)])
            rowval = np.where(c.perm >= E_, c.perm - E_, c.perm)       # a mirrored position reads the row of the edge it mirrors
            dt = np.int64 if ib == 8 else np.int32

            def ref(host, c=c, tot=tot, colptr=colptr, rowval=rowval, ib=ib, base=base):
                assert host["total"] == tot, (host["total"], tot)
                I = lambda v, b: E((np.asarray(v, np.int64) + b).astype(np.int64 if ib == 8 else np.int32), "exact", prefix=len(v))      # noqa: E731
                return {"s_out": I(c.s - 1, base), "t_out": I(c.t - 1, base), "colptr": I(colptr, base), "rowval": I(rowval, base)}
            job = Rec("gnnmp_coalesce_t", s=Arr("s", "in", IX(s1, ib, base)), t=Arr("t", "in", IX(t1, ib, base)), idx_bytes=ib, index_base=base, n_edges=E_, n_nodes=n,
                      mode=mode, s_out=Arr("s_out", "out", shape=(Ev,), dtype=dt), t_out=Arr("t_out", "out", shape=(Ev,), dtype=dt),
                      colptr=Arr("colptr", "out", shape=(Ev + 1,), dtype=dt), rowval=Arr("rowval", "out", shape=(Ev,), dtype=dt))
            yield mk("gnnmp_coalesce_edges", f"n{n}_E{E_}_m{mode}_i{ib}b{base}", ({"align"} if n in (31, 33) else set()) | ({"side"} if k == 4 else set()),
                     [job, HostOut("total"), STREAM], ref)
            k += 1


@cases_of("gnnmp_compact_edges")
def _(ctx):
    TR = _mod("transforms_ref")
    k = 0
    for n, E_ in PREP[:4]:
        for rule in (0, 1, 2):                                          # SELF_LOOPS, LIST, RANDOM
            ib, base = IDX[k % 4]
            r = rng_of("compact", n, E_, rule)
            s1, t1 = r.integers(1, n + 1, E_), r.integers(1, n + 1, E_)
            t1[::3] = s1[::3]                                           # self loops
            w = F(r, E_) if k % 2 == 0 else None
            rem = r.integers(1, E_ + 1, max(1, E_ // 3))                # 1-based positions, repeats allowed
            pdrop, seed = 0.4, 99 + k
            if rule == 0:
                keep = np.flatnonzero(s1 != t1)
                assert np.array_equal(keep, TR.remove_self_loops(s1, t1)[4])
            elif rule == 1:
                keep = TR.remove_edges(s1, t1, rem)[4]
            else:                                                       # the hash of gnnmp_dropout_keep_u8 at (seed, e, h = 0): the oracle's mask
                keep = np.flatnonzero(np.asarray(orc().dropout_keep(seed, pdrop, E_, 1)).reshape(E_) != 0)
            tot = len(keep)
            dt = np.int64 if ib == 8 else np.int32

            def ref(host, keep=keep, s1=s1, t1=t1, w=w, tot=tot, ib=ib, base=base):
                assert host["total"] == tot, (host["total"], tot)
                I = lambda v: E((np.asarray(v, np.int64) + base).astype(np.int64 if ib == 8 else np.int32), "exact", prefix=len(v))      # noqa: E731
                out = {"s_out": I(s1[keep] - 1), "t_out": I(t1[keep] - 1), "eid_out": I(keep)}
                if w is not None:
                    out["w_out"] = E(w[keep], "exact", prefix=tot)
                return out
            job = Rec("gnnmp_compact_t", s=Arr("s", "in", IX(s1, ib, base)), t=Arr("t", "in", IX(t1, ib, base)), w=Arr("w", "in", w) if w is not None else None,
                      idx_bytes=ib, index_base=base, n_edges=E_, rule=rule, remove=Arr("remove", "in", IX(rem, ib, base)) if rule == 1 else None,
                      n_remove=len(rem) if rule == 1 else 0, p=pdrop, seed=seed, s_out=Arr("s_out", "out", shape=(E_,), dtype=dt),
                      t_out=Arr("t_out", "out", shape=(E_,), dtype=dt), w_out=Arr("w_out", "out", shape=(E_,)) if w is not None else None,
                      eid_out=Arr("eid_out", "out", shape=(E_,), dtype=dt))
            yield mk("gnnmp_compact_edges", f"n{n}_E{E_}_r{rule}_i{ib}b{base}", ({"align"} if n in (31, 33) else set()) | ({"side"} if k == 4 else set()),
                     [job, HostOut("total"), STREAM], ref)
            k += 1


@cases_of("gnnmp_random_walk_pe_f32")
def _(ctx):
    W = _mod("rwpe_ref")
    T = 16                                                              # GNNMP_RWPE_TILE: members of T - 1, T, T + 1 and 2 T + 1 nodes
    if "rwpe" not in ctx.cache:
        (bs, bt, bn, _), off = W.concat(W.batch_members(T))
        ls, lt, ln, _ = W.random_graph(520, 3, 300)                    # more nodes than the LDS panels hold: the scratch path
        ctx.cache["rwpe"] = (Graph("rwpe_batch", bs + 1, bt + 1, bn), off, Graph("rwpe_520", ls + 1, lt + 1, ln))
    gbatch, off, glarge = ctx.cache["rwpe"]
    shapes = [(ctx.hub, 6, None, {"align", "side", "ws"}), (ctx.e0, 3, None, ()), (ctx.one, 4, None, ()), (ctx.r31, 1, None, {"align"}), (ctx.r33, 5, None, ()),
              (ctx.r300, 6, None, ()), (gbatch, W.BATCH_WALK, 8, ()), (gbatch, 3, 4, {"align"}), (glarge, 3, None, ())]
    for k, (g, K, pb, tags) in enumerate(shapes):
        r = rng_of("rwpe", g.name, K, pb)
        w = (1.0 + 0.5 * F(r, g.E)).astype(f32)
        with_w = k % 2 == 0
        pe = W.dense64(g.s - 1, g.t - 1, g.n, w if with_w else None, K)
        # tests/test_rwpe.py's bar: 1e-5 norm-wise AND element-wise relative, and exactly 0 where the model is 0
        ref = lambda host, pe=pe: {"out": E(pred=lambda got, pe=pe: None if W.within_bar(got, pe) else "deviation %r from float64 is not within 1e-5" % (W.deviation(got, pe),))}
        job = Rec("gnnmp_rwpe_t", w=Arr("w", "in", w) if with_w else None, graph_ptr=Arr("graph_ptr", "in", off.astype(np.int64 if pb == 8 else np.int32)) if pb else None,
                  idx_bytes=pb or 8, n_graphs=len(off) - 1 if pb else 1, walk_length=K, out=Arr("out", "out", shape=(g.n, K)))
        yield mk("gnnmp_random_walk_pe_f32", f"{g.name}_K{K}_w{int(with_w)}_p{pb or 0}", tags, [Pl(g, T=True), job, STREAM], ref)


@cases_of("gnnmp_gmm_weights_grad_f32")
def _(ctx):
    G = _mod("gmm_conv_ref")
    for k, (E_, ein, K) in enumerate(G.WGRAD_CASES):                    # E = 1, 7, 257 and three slices and a remainder a block
        how = (("de", "par"), ("par",), ("de",))[k % 3]
        r = rng_of("gmm_weights_grad", E_, ein, K)
        e = F(r, E_, ein)
        sc = np.sqrt(6.0 / (K + ein))
        mu, sinv = (sc * F(r, K, ein)).astype(f32), (sc * F(r, K, ein)).astype(f32)
        w, dw = G.weights(e, mu, sinv), F(r, E_, K)
        de64, dmu64, dsinv64, mag_mu, mag_s = G.wgrad64(e, mu, sinv, w, dw)

        def bounded(v, mag, E_=E_):                                    # tests/test_gmm_conv_ad.py: the fp32 summation bound at the documented fold depth
            return E(pred=lambda got: None if np.all(np.abs(got.astype(f64) - v) <= G.sum_bound(E_, mag)) else "outside the summation bound")

        def ref(host, how=how, v=(de64, dmu64, dsinv64, mag_mu, mag_s)):
            out = {"de": E(v[0])} if "de" in how else {}
            if "par" in how:
                out.update(dmu=bounded(v[1], v[3]), dsinv=bounded(v[2], v[4]),
                           part=E(pred=lambda got: None if np.all(np.isfinite(got)) else "non-finite partials"))      # every element written: the slab's check
            return out
        par = "par" in how
        job = Rec("gnnmp_gmm_weights_grad_t", e=Arr("e", "in", e), mu=Arr("mu", "in", mu), sinv=Arr("sinv", "in", sinv), w=Arr("w", "in", w), dw=Arr("dw", "in", dw),
                  de=Arr("de", "out", shape=(E_, ein)) if "de" in how else None, dmu=Arr("dmu", "out", shape=(K, ein)) if par else None,
                  dsinv=Arr("dsinv", "out", shape=(K, ein)) if par else None, part=Arr("part", "out", shape=(G.PARTS, 2, K, ein)) if par else None)
        yield mk("gnnmp_gmm_weights_grad_f32", f"E{E_}_ein{ein}_K{K}_{'_'.join(how)}", ({"align"} if k in (4, 9, 11) else set()) | ({"side"} if k == 0 else set()),
                 [job, E_, ein, K, STREAM], ref, no_warmup=True)


# ---- the GraphConv chain: graph_chain_kernel (csrc/graph_chain.hip) and the wave-pair kernel (csrc/graph_chain2.hip) ---------------------
KNOB_CHAIN = 18                      # csrc/knobs.h: 1 = the general kernel only
CHAIN_ALIGN = {"x": EUNSUPPORTED, "scratch": EUNSUPPORTED}      # include/gnnmp.h: x and scratch are 16-byte aligned, or the call refuses


def chain_scratch_floats(N, dims, nout):
    """gnnmp_graphconv_chain_scratch_floats(N, n_layers, dims, nout), asked of the library: the scratch array of a case has EXACTLY that many
    floats, so the slab's guard bands say whether the number is enough.  Outside the function's domain (-1: more than four layers) a
    refusal case gets a token array.  Without a loadable library (a dry run of the table before the build) the header's layout is
    restated: the widest layer of each of the two buffers, the z rows, 16 floats of padding"""
    nl = len(dims) - 1
    try:
        from gnnmp import _lib
        need = int(_lib.load().gnnmp_graphconv_chain_scratch_floats(N, nl, (ctypes.c_int64 * (nl + 1))(*dims), nout))
    except (ImportError, OSError):
        need = N * (max(dims[1::2]) + max(dims[2::2], default=0) + nout) + 16 if nl <= 4 else -1
    return need if need > 0 else 64


def chain_batch(ctx, name, sizes, seed, hub=None):
    """(graph, seg_ptr) of a batch of member graphs of `sizes` nodes (0: an empty member), made once per Ctx: random directed edges inside
    each member (multi-edges and self edges as they fall), the last node of every member of five nodes and more isolated, the edge list
    shuffled; hub = (member, node, k): k more in-edges for that node"""
    if ("chain", name) not in ctx.cache:
        rng = np.random.default_rng(seed)
        seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        ss, tt = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
        for k, n in enumerate(sizes):
            if n < 2:
                continue
            m = int(rng.integers(n, 3 * n + 1))
            s, t = rng.integers(0, n, m), rng.integers(0, n, m)
            if n >= 5:
                s, t = s[t != n - 1], t[t != n - 1]
            ss.append(s + seg[k])
            tt.append(t + seg[k])
        if hub is not None:
            k, node, cnt = hub
            ss.append(rng.integers(0, sizes[k], cnt) + seg[k])
            tt.append(np.full(cnt, node + seg[k]))
        s, t = np.concatenate(ss), np.concatenate(tt)
        perm = rng.permutation(len(s))
        ctx.cache["chain", name] = (Graph("chain_" + name, s[perm] + 1, t[perm] + 1, int(seg[-1])), seg)
    return ctx.cache["chain", name]


def chain_ref64(g, seg, x, layers, aggr, pool, Wh, bh):
    """float64: per layer act(W_root x_i + W_agg aggr_j x_j + b), pooled per member graph, then the head.  layers: [(W_root, W_agg, bias |
    None, act)] with W (dout, din); Wh (nout, dL).  Returns (logits [G][nout], scale [G][nout] = Σ_c |Wh(o, c) p_c| + |b_o|: what a
    logit's rounding error lives on when its terms cancel)"""
    s0, t0, N = g.s - 1, g.t - 1, g.n_dst
    deg = np.bincount(t0, minlength=N).astype(f64)
    h = np.asarray(x, f64)
    with np.errstate(invalid="ignore"):
        for Wr, Wa, b, a in layers:
            m = seg_sum(t0, h[s0], N)
            if aggr == MEAN:
                m = m / np.maximum(deg, 1.0)[:, None]
            z = h @ np.asarray(Wr, f64).T + m @ np.asarray(Wa, f64).T
            h = act64(a, z if b is None else z + np.asarray(b, f64))
        G = len(seg) - 1
        p = np.zeros((G, h.shape[1]), f64)
        for k in range(G):
            rows = h[seg[k]:seg[k + 1]]
            if len(rows):
                p[k] = rows.sum(0) / (len(rows) if pool == MEAN else 1)
        terms = np.asarray(Wh, f64)[None, :, :] * p[:, None, :]
        b64 = np.zeros(len(Wh), f64) if bh is None else np.asarray(bh, f64)
        logits, scale = terms.sum(-1) + b64, np.abs(terms).sum(-1) + np.abs(b64)
    return logits, np.where(np.isfinite(scale), scale, 0.0)


def _chain_case(ctx, sid, tags, g, seg, dims, nout, aggr, pool, lay=0, acts=None, bias="all", b_head=True, jobs=None, nan_member=None,
                knobs=None, status=OK, n_layers=None, w_layout=None, salt=()):
    """one call of gnnmp_graphconv_chain_f32.  dims, acts, nout, aggr, pool, w_layout go to the library as given (a refusal case gives
    what the library must refuse); lay in (0, 1) is how the weights are STORED.  bias: 'all' | 'none' (the table itself is NULL) | the
    layer whose entry is NULL.  salt: added to the key of the float draws (two cases of one sid-independent operand set share it)"""
    N, G = g.n_dst, len(seg) - 1
    nl = len(dims) - 1
    acts = tuple(acts) if acts is not None else (1,) * nl
    r = rng_of("chain", *(salt or (sid,)))
    x = F(r, N, dims[0])
    store = (lambda W: np.ascontiguousarray(W.T)) if lay else (lambda W: W)
    layers, Wr_a, Wa_a, b_a = [], [], [], []
    for l in range(nl):
        din, dout = dims[l], dims[l + 1]
        Wr, Wa = F(r, dout, din) * f32(1.0 / np.sqrt(din)), F(r, dout, din) * f32(1.0 / np.sqrt(din))
        b = F(r, dout) * f32(0.5)
        has_b = bias == "all" or (bias != "none" and bias != l)
        layers.append((Wr, Wa, b if has_b else None, acts[l]))
        Wr_a.append(Arr(f"W_root{l}", "in", store(Wr)))
        Wa_a.append(Arr(f"W_agg{l}", "in", store(Wa)))
        b_a.append(Arr(f"bias{l}", "in", b) if has_b else None)
    Wh, bh = F(r, nout, dims[-1]) * f32(1.0 / np.sqrt(dims[-1])), F(r, nout) * f32(0.5)
    if nan_member is not None:                            # one feature of the member's first node: every logit of that member is NaN, no other
        x[seg[nan_member], 1] = np.nan
    ref = None
    if status == OK:
        def ref(host, v=(g, seg, x, layers, aggr, pool, Wh, bh if b_head else None)):
            logits, scale = chain_ref64(*v)
            return {"out": E(logits, scale=scale)}
    args = [Pl(g), jobs or Jobs("none"), Arr("seg_ptr", "in", seg), G, Arr("x", "in", x), nl if n_layers is None else n_layers,
            HostArr(ctypes.c_int64, dims), PtrTab(Wr_a), PtrTab(Wa_a), None if bias == "none" else PtrTab(b_a), HostArr(ctypes.c_int, acts),
            lay if w_layout is None else w_layout, aggr, pool, Arr("W_head", "in", store(Wh)), Arr("b_head", "in", bh) if b_head else None, nout,
            Arr("scratch", "scratch", shape=(chain_scratch_floats(N, dims, nout),)), Arr("out", "out", shape=(G, nout)), STREAM]
    return mk("gnnmp_graphconv_chain_f32", sid, tags, args, ref, status=status, align_status=CHAIN_ALIGN, knobs=knobs)


CHAIN_PAIR_SIZES = ([64], [32], [33, 31], [64, 64, 1], [2, 63, 17, 47, 64, 1, 1, 30])      # tests/test_graph_chain.py: the job shapes at the pair kernel's edges


@cases_of("gnnmp_graphconv_chain_f32")
def _(ctx):
    C = lambda *a, **k: _chain_case(ctx, *a, **k)
    # ---- the general kernel: jobs NULL ---------------------------------------------------------------------------------------------------
    # 303 rows in 12 members of 1 .. 70 nodes (one above 64), two blocks (N / 128), node 3 of member 0 with 200 more in-edges (past the
    # four prefetched neighbour pointers, and a split row of the plan), isolated nodes
    big, bseg = chain_batch(ctx, "big", [70, 1, 33, 20, 5, 40, 17, 64, 2, 29, 12, 10], 41, hub=(0, 3, 200))
    yield C("big_16x128x128_sum_mean_n2", {"align", "ws"}, big, bseg, (16, 128, 128), 2, SUM, MEAN)      # Pass<16>, the two-part Pass<128>, FULLCOLS
    yield C("big_8x32_mean_sum_n1", (), big, bseg, (8, 32), 1, MEAN, SUM, acts=(0,))                      # one layer: never stored, d1 = 0; run-time Din
    yield C("big_20x64x8x128_sum_sum_n3", (), big, bseg, (20, 64, 8, 128), 3, SUM, SUM)                   # Din % 16 != 0; a stored layer of 8 columns; h[0] shared
    yield C("big_4x8x8x8x4_lay1_nobias_n8", (), big, bseg, (4, 8, 8, 8, 4), 8, MEAN, MEAN, lay=1, bias="none", b_head=False, acts=(1, 0, 1, 0))
    yield C("big_4x8x8x8x4_lay1_bias2null_n8", (), big, bseg, (4, 8, 8, 8, 4), 8, SUM, MEAN, lay=1, bias=2, acts=(1, 0, 1, 0))
    yield C("big_16x128x128_nan_member5", (), big, bseg, (16, 128, 128), 2, SUM, MEAN, nan_member=5)
    # empty member graphs, first, interior (two in a row) and last: their rows of `out` are b_head
    emp, eseg = chain_batch(ctx, "empty", [0, 20, 0, 0, 30, 14, 0], 42)
    yield C("empty_16x64_mean_mean_n3", (), emp, eseg, (16, 64), 3, MEAN, MEAN)
    yield C("empty_16x128x128_sum_sum_n2", (), emp, eseg, (16, 128, 128), 2, SUM, SUM)
    yield C("empty_16x128x128_sum_sum_nobhead", (), emp, eseg, (16, 128, 128), 2, SUM, SUM, b_head=False)
    n32, s32 = chain_batch(ctx, "n32", [32], 43)
    n33, s33 = chain_batch(ctx, "n33", [20, 13], 44)
    yield C("n32_G1_12x16_sum_mean_n2", (), n32, s32, (12, 16), 2, SUM, MEAN)
    yield C("n33_12x16x8_mean_sum_n5", (), n33, s33, (12, 16, 8), 5, MEAN, SUM)
    # ---- refusals: nothing may be written ---------------------------------------------------------------------------------------------------
    n31, s31 = chain_batch(ctx, "n31", [31], 45)
    U = dict(status=EUNSUPPORTED)
    yield C("refuse_N31", (), n31, s31, (16, 128), 2, SUM, MEAN, **U)
    yield C("refuse_dout132", (), n33, s33, (16, 132), 2, SUM, MEAN, **U)
    yield C("refuse_din6", (), n33, s33, (6, 16), 2, SUM, MEAN, **U)
    yield C("refuse_stored_dout4", (), n33, s33, (16, 4, 8), 2, SUM, MEAN, **U)
    yield C("refuse_aggr_max", (), n33, s33, (16, 16), 2, MAX, MEAN, **U)
    yield C("refuse_pool_max", (), n33, s33, (16, 16), 2, SUM, MAX, **U)
    yield C("refuse_nout9", (), n33, s33, (16, 16), 9, SUM, MEAN, **U)
    yield C("refuse_5_layers", (), n33, s33, (8, 8, 8, 8, 8, 8), 2, SUM, MEAN, **U)
    yield C("refuse_act_tanh", (), n33, s33, (16, 16), 2, SUM, MEAN, acts=(3,), **U)
    yield C("refuse_w_layout2", (), n33, s33, (16, 16), 2, SUM, MEAN, w_layout=2, status=EINVAL)
    if ("chain", "nonsquare") not in ctx.cache:
        ctx.cache["chain", "nonsquare"] = random_graph("chain_nonsquare", 40, 90, 46, n_dst=33)
    yield C("refuse_nonsquare_plan", (), ctx.cache["chain", "nonsquare"], s33, (16, 16), 2, SUM, MEAN, status=EINVAL)
    # ---- the wave-pair kernel: (16, 128, 128), members of at most 64 nodes, a jobs handle packed on the host and on the device ---------------
    # each operand set runs three times on the same values (the salt): host-packed jobs, device-packed jobs — bit-equal, asserted in
    # tests/test_abi_memory_contract.py — and the general kernel (KNOB_CHAIN = 1), all against the float64 reference
    heads = ((1, SUM, MEAN, 0), (3, MEAN, SUM, 1), (8, SUM, MEAN, 1), (2, MEAN, SUM, 0), (3, SUM, MEAN, 0))      # nout, aggr, pool, layout
    for k, (sizes, (nout, aggr, pool, lay)) in enumerate(zip(CHAIN_PAIR_SIZES, heads)):
        name = "-".join(map(str, sizes))
        g, seg = chain_batch(ctx, "pair_" + name, sizes, 50 + k)
        what = f"pair_{name}_n{nout}_{'sum' if aggr == SUM else 'mean'}_lay{lay}"
        for mode in ("host", "device"):
            tags = {"side"} if (k, mode) == (4, "host") else {"align", "ws"} if (k, mode) == (4, "device") else ()
            yield C(f"{what}_{mode}", tags, g, seg, (16, 128, 128), nout, aggr, pool, lay=lay, jobs=Jobs(mode, seg), salt=(what,))
        yield C(f"{what}_general", (), g, seg, (16, 128, 128), nout, aggr, pool, lay=lay, jobs=Jobs("host", seg), salt=(what,), knobs={KNOB_CHAIN: 1})
    # a NaN member: its job is set aside for the exact path; then the SAME handle on finite values (the device re-armed the counter)
    g, seg = chain_batch(ctx, "pair_" + "-".join(map(str, CHAIN_PAIR_SIZES[4])), CHAIN_PAIR_SIZES[4], 54)
    for mode in ("host", "device"):
        yield C(f"pair_nan_member2_{mode}", (), g, seg, (16, 128, 128), 2, SUM, MEAN, jobs=Jobs(mode, seg), nan_member=2, salt=("pair_nan",))
        yield C(f"pair_finite_after_nan_{mode}", (), g, seg, (16, 128, 128), 2, SUM, MEAN, jobs=Jobs(mode, seg), salt=("pair_finite",))
    # a handle the pair kernel must decline: it has no jobs (an empty member; a member above 64 nodes), the general kernel runs
    for mode in ("host", "device"):
        yield C(f"declined_empty_member_{mode}", (), emp, eseg, (16, 128, 128), 2, SUM, MEAN, jobs=Jobs(mode, eseg))
        yield C(f"declined_member_of_70_{mode}", (), big, bseg, (16, 128, 128), 2, MEAN, SUM, jobs=Jobs(mode, bseg))


# ------------------------------------------------------------------------------------------------------------------------------------
# PREP_TABLE: the writers that synchronise — plan export, the plans of a batch (csrc/plan_batch.hip), the plans of an edited graph
# (csrc/plan_edit.hip), the job table of the wave-pair chain kernel.  The same Case objects and the same slab; they are graph prep, not
# recordable, so tests/test_abi_graph_capture.py and the lane-group sweep leave them alone.  Every reference is exact.
# ------------------------------------------------------------------------------------------------------------------------------------
PREP_TABLE = {}


def prep_cases_of(export):
    def deco(fn):
        PREP_TABLE[export] = fn
        return fn
    return deco


def csr_of(s1, t1, n, loops):
    """(rowptr, col, eid) of gnnmp_plan_create on the 1-based COO (s1, t1) over n nodes: slots in destination order, stable in the edge
    position; a plan-added self loop is edge E + node (it sorts to the end of its row).  All 0-based"""
    s0, t0 = np.asarray(s1, np.int64) - 1, np.asarray(t1, np.int64) - 1
    if loops:
        s0, t0 = np.concatenate([s0, np.arange(n)]), np.concatenate([t0, np.arange(n)])
    order = np.argsort(t0, kind="stable")
    return np.concatenate([[0], np.cumsum(np.bincount(t0, minlength=n))]), s0[order], order


def batch_of(members):
    """MLUtils.batch of Graph members: (s, t) 1-based with the nodes offset member after member, node offsets"""
    off = np.concatenate([[0], np.cumsum([m.n for m in members])]).astype(np.int64)
    s = np.concatenate([np.zeros(0, np.int64)] + [m.s + off[k] for k, m in enumerate(members)])
    t = np.concatenate([np.zeros(0, np.int64)] + [m.t + off[k] for k, m in enumerate(members)])
    return s, t, off


def _csr_arrays(n, tot, wide=False, prefix=""):
    """the three outputs of gnnmp_plan_export(64) of a plan of n rows and tot slots (an array of no element is passed as NULL)"""
    return [Arr(prefix + "rowptr", "out", shape=(n + 1,), dtype=np.int64 if wide else np.int32, field="rowptr"),
            Arr(prefix + "col", "out", shape=(tot,), dtype=np.int32, field="col") if tot else None,
            Arr(prefix + "eid", "out", shape=(tot,), dtype=np.uint32 if wide else np.int32, field="eid") if tot else None]


def _csr_ref(csr, prefix=""):
    rowptr, col, eid = csr
    return {prefix + "rowptr": E(rowptr, "exact"), **({prefix + "col": E(col, "exact"), prefix + "eid": E(eid, "exact")} if len(col) else {})}


def _exported(n, csr):
    """Case.then: gnnmp_plan_export of the plan the call created, into the slab"""
    return ("gnnmp_plan_export", [Made("plan")] + _csr_arrays(n, len(csr[1]), prefix="new_") + [STREAM])


def _ctx_graphs(ctx):
    return (ctx.hub, ctx.e0, ctx.one, ctx.r31, ctx.r33, ctx.r300)


def _plan_export(export, wide):
    def build(ctx):
        for g in _ctx_graphs(ctx):
            for loops in (False, True):
                csr = csr_of(g.s, g.t, g.n, loops)
                tags = {"align", "side"} if (g is ctx.hub and not loops) else {"align"} if (g is ctx.r33 and loops) else ()
                yield mk(export, f"{g.name}_loops{int(loops)}", tags, [Pl(g, loops=loops)] + _csr_arrays(g.n, len(csr[1]), wide) + [STREAM],
                         lambda host, csr=csr: _csr_ref(csr))
        g = ctx.r31                                                    # "any may be NULL": each output alone
        csr = csr_of(g.s, g.t, g.n, False)
        for k, name in enumerate(("rowptr", "col", "eid")):
            arrs = [a if a.field == name else None for a in _csr_arrays(g.n, len(csr[1]), wide)]
            yield mk(export, f"{g.name}_only_{name}", (), [Pl(g)] + arrs + [STREAM], lambda host, name=name, v=csr[k]: {name: E(v, "exact")})
    return build


PREP_TABLE["gnnmp_plan_export"] = _plan_export("gnnmp_plan_export", False)
PREP_TABLE["gnnmp_plan_export64"] = _plan_export("gnnmp_plan_export64", True)


@prep_cases_of("gnnmp_plan_edge_index")
def _(ctx):
    k = 0
    for g in _ctx_graphs(ctx):
        for loops in (False, True):
            for ib, base in (IDX if g is ctx.r33 else (IDX[k % 4],)):
                k += 1
                dt = np.int64 if ib == 8 else np.int32
                tags = {"align", "side"} if (g is ctx.hub and not loops) else {"align"} if (g is ctx.r33 and loops) else ()
                outs = [Arr("out_src", "out", shape=(g.E,), dtype=dt), Arr("out_dst", "out", shape=(g.E,), dtype=dt)] if g.E else [None, None]
                yield mk("gnnmp_plan_edge_index", f"{g.name}_loops{int(loops)}_i{ib}b{base}", tags, [Pl(g, loops=loops), ib, base] + outs + [STREAM],
                         lambda host, g=g, ib=ib, base=base: {"out_src": E(IX(g.s, ib, base), "exact"), "out_dst": E(IX(g.t, ib, base), "exact")} if g.E else {})


def _prep_members(ctx):
    """six member graphs of a dataset: one without edges, one of a single node with a self edge"""
    if "prep_members" not in ctx.cache:
        ctx.cache["prep_members"] = [random_graph("m0", 5, 12, 61), Graph("m1", [], [], 4), Graph("m2", [1], [1], 1), random_graph("m3", 33, 100, 62),
                                     random_graph("m4", 7, 20, 63), random_graph("m5", 12, 30, 64)]
    return ctx.cache["prep_members"]


def _batch_outputs(members, ib, base, want_seg, want_ind, node_ptr=None, ids=None):
    """(arrays, reference) of the optional outputs of gnnmp_plan_concat / gnnmp_plan_select for the batch `members` (select: the dataset's
    node offsets and the chosen ids, which add node_map_out)"""
    s, t, off = batch_of(members)
    N, dt = int(off[-1]), np.int64 if ib == 8 else np.int32
    arrs = [Arr("seg_ptr_out", "out", shape=(len(members) + 1,), dtype=np.int64) if want_seg else None]
    ref = {"seg_ptr_out": E(off, "exact")} if want_seg else {}
    if node_ptr is not None:
        want_map = want_ind or not want_seg      # (each of the three is NULL in some case; node_map_out is the only output in one)
        arrs.append(Arr("node_map_out", "out", shape=(N,), dtype=np.int32) if want_map else None)
        if want_map:
            ref["node_map_out"] = E(np.concatenate([np.arange(node_ptr[i], node_ptr[i + 1]) for i in ids]), "exact")
    arrs.append(Arr("graph_indicator_out", "out", shape=(N,), dtype=dt) if want_ind else None)
    if want_ind:
        ref["graph_indicator_out"] = E(IX(np.repeat(np.arange(1, len(members) + 1), [m.n for m in members]), ib, base), "exact")
    return arrs, ref, (s, t, N)


# (self loops, members in batch order — with a repeat where the call allows it —, seg_ptr_out, graph_indicator_out, its width and base)
PREP_BATCHES = ((False, (0, 1, 2, 3), True, True, 8, 1, {"align", "side"}), (True, (3, 1, 0, 2), True, True, 4, 0, {"align"}), (False, (1, 0, 3), False, True, 4, 1, ()),
                (True, (2, 3, 1, 0), True, False, 8, 0, ()), (False, (3, 0, 5, 1), False, False, 8, 1, ()), (True, (5, 4, 2), True, True, 8, 0, ()))


@prep_cases_of("gnnmp_plan_concat")
def _(ctx):
    M = _prep_members(ctx)
    for loops, order, want_seg, want_ind, ib, base, tags in PREP_BATCHES:
        members = [M[i] for i in order]
        arrs, ref, (s, t, N) = _batch_outputs(members, ib, base, want_seg, want_ind)
        csr = csr_of(s, t, N, loops)
        yield mk("gnnmp_plan_concat", f"loops{int(loops)}_{''.join(map(str, order))}_seg{int(want_seg)}_ind{int(want_ind)}_i{ib}b{base}", tags,
                 [NewPlan("plan"), PlanTab([Pl(m, loops=loops) for m in members]), len(members)] + arrs + [ib, base, STREAM],
                 lambda host, ref=ref, csr=csr: {**ref, **_csr_ref(csr, "new_")}, then=_exported(N, csr))


@prep_cases_of("gnnmp_plan_select")
def _(ctx):
    M = _prep_members(ctx)
    if "prep_dataset" not in ctx.cache:
        s, t, off = batch_of(M)                                         # member-major, as MLUtils.batch makes it
        ctx.cache["prep_dataset"] = (Graph("prep_dataset", s, t, int(off[-1])), off)
    ds, node_ptr = ctx.cache["prep_dataset"]
    for loops, order, want_seg, want_ind, ib, base, tags in PREP_BATCHES:
        ids = list(order) + [order[0]]                                   # batch(gs[ids]) takes any index vector: one id twice
        members = [M[i] for i in ids]
        arrs, ref, (s, t, N) = _batch_outputs(members, ib, base, want_seg, want_ind, node_ptr, ids)
        csr = csr_of(s, t, N, loops)
        yield mk("gnnmp_plan_select", f"loops{int(loops)}_{''.join(map(str, ids))}_seg{int(want_seg)}_ind{int(want_ind)}_i{ib}b{base}", tags,
                 [NewPlan("plan"), Pl(ds, loops=loops), Arr("node_ptr", "in", node_ptr), len(M), Arr("ids", "in", IX(np.asarray(ids) + 1, ib, base)), ib, base,
                  len(ids), N, len(csr[1])] + arrs + [STREAM],
                 lambda host, ref=ref, csr=csr: {**ref, **_csr_ref(csr, "new_")}, then=_exported(N, csr))


def _totals(host, n_keep, e_keep):
    assert list(host["total"]) == [n_keep, e_keep], (list(host["total"]), [n_keep, e_keep])


@prep_cases_of("gnnmp_plan_remove_nodes")
def _(ctx):
    R = _mod("augment_ref")
    # (graph, self loops, what goes: a descending list with repeats | a probability of the restated node mask, the optional outputs)
    shapes = ((ctx.r33, False, "list", True, {"align", "side"}), (ctx.r300, True, "list", True, {"align"}), (ctx.r31, True, "list", False, ()),
              (ctx.r300, False, 0.3, True, ()), (ctx.r33, True, 0.5, True, ()), (ctx.hub, False, "list", True, ()))
    for k, (g, loops, what, maps, tags) in enumerate(shapes):
        ib, base = IDX[k % 4]
        s0, t0, N = g.s - 1, g.t - 1, g.n
        if what == "list":
            pick = rng_of("remove_nodes", g.name).permutation(N)[: max(1, N // 4)]
            lst = np.sort(np.concatenate([pick, pick[: max(1, len(pick) // 2)]]))[::-1]
            s2, t2, _, n2, nid, eid = R.remove_nodes(s0, t0, None, N, lst, base=0)
            head = [Arr("remove", "in", IX(lst + 1, ib, base)), ib, base, len(lst), 0.0, 0]
        else:
            seed = 0xDEADBEEF12345 + k
            s2, t2, _, n2, nid, eid = R.remove_nodes_p(s0, t0, None, N, what, seed, base=0)
            head = [None, ib, base, 0, what, seed]
        assert 0 < n2 < N and len(s2) > 0
        new = np.full(N, -1, np.int64)
        new[nid] = np.arange(n2)
        csr = csr_of(s2 + 1, t2 + 1, n2, loops)
        outs = [Arr("node_map_out", "out", shape=(n2,), dtype=np.int32), Arr("node_new_out", "out", shape=(N,), dtype=np.int32),
                Arr("edge_map_out", "out", shape=(len(s2),), dtype=np.uint32)] if maps else [None, None, None]
        def ref(host, v=(n2, len(s2), nid, new, eid, csr), maps=maps):
            _totals(host, v[0], v[1])
            out = {"node_map_out": E(v[2], "exact"), "node_new_out": E(v[3], "exact"), "edge_map_out": E(v[4], "exact")} if maps else {}
            return {**out, **_csr_ref(v[5], "new_")}
        yield mk("gnnmp_plan_remove_nodes", f"{g.name}_loops{int(loops)}_{what}_maps{int(maps)}_i{ib}b{base}", tags,
                 [NewPlan("plan"), Pl(g, loops=loops)] + head + outs + [HostOut("total", ctypes.c_int64 * 2), STREAM], ref, then=_exported(n2, csr))


@prep_cases_of("gnnmp_plan_add_edges")
def _(ctx):
    R = _mod("augment_ref")
    # (graph, self loops, new edges, nodes of the child, list mode | the restated pair draw)
    shapes = ((ctx.r33, False, 40, 38, "list", {"align", "side"}), (ctx.r300, True, 77, 300, "draw", {"align"}), (ctx.r31, True, 1, 31, "list", ()),
              (ctx.r33, True, 33, 33, "draw", ()), (ctx.r300, False, 907, 309, "list", ()), (ctx.e0, False, 9, 5, "draw", ()))
    for k, (g, loops, m, n_nodes, mode, tags) in enumerate(shapes):
        ib, base = IDX[k % 4]
        dt = np.int64 if ib == 8 else np.int32
        seed = (k << 40) + 99
        if mode == "list":
            r = rng_of("add_edges", g.name, m)
            sn, tn = r.integers(0, n_nodes, m), r.integers(0, n_nodes, m)
            mid = [Arr("s_new", "in", IX(sn + 1, ib, base)), Arr("t_new", "in", IX(tn + 1, ib, base)), ib, base, m, n_nodes, 0, None, None]
        else:
            sn, tn = R.rand_pairs(seed, m, g.n)
            mid = [None, None, ib, base, m, n_nodes, seed, Arr("s_new_out", "out", shape=(m,), dtype=dt), Arr("t_new_out", "out", shape=(m,), dtype=dt)]
        csr = csr_of(np.concatenate([g.s, sn + 1]), np.concatenate([g.t, tn + 1]), n_nodes, loops)
        def ref(host, sn=sn, tn=tn, csr=csr, mode=mode, ib=ib, base=base):
            out = {"s_new_out": E(IX(sn + 1, ib, base), "exact"), "t_new_out": E(IX(tn + 1, ib, base), "exact")} if mode == "draw" else {}
            return {**out, **_csr_ref(csr, "new_")}
        yield mk("gnnmp_plan_add_edges", f"{g.name}_loops{int(loops)}_m{m}_n{n_nodes}_{mode}_i{ib}b{base}", tags,
                 [NewPlan("plan"), Pl(g, loops=loops)] + mid + [STREAM], ref, then=_exported(n_nodes, csr))


def bfd_jobs(sizes):
    """the number of jobs of gnnmp_chain_jobs_create: best fit decreasing into jobs of 64 rows (members by decreasing size, ties by id,
    each into the fullest job that still takes it)"""
    room = []
    for sz in sorted((int(v) for v in sizes if v > 0), reverse=True):
        fits = [j for j, r in enumerate(room) if r >= sz]
        if fits:
            room[min(fits, key=lambda j: room[j])] -= sz
        else:
            room.append(64 - sz)
    return len(room)


def _job_table_ref(sizes, njobs, mode):
    """what gnnmp_chain_jobs_export owes (tests/test_plan_batch.py: check_packing, tests/test_graph_chain.py: test_job_packing): every row of
    the batch in exactly one slot, members whole, contiguous and in node order, a job filled from slot 0 without holes and of at most 64
    rows, -1 in every other slot — the header: a row at or above the job count holds -1 throughout.  hdr_out[0..4] exactly: jobs, 32-row
    tiles (counted on the exported table; 0 from a host-packed handle), not poisoned, the largest member, the empty members.  The phase
    stamps hdr_out[16..29] are timings: written, not compared"""
    sizes = np.asarray(sizes, np.int64)
    seg = np.concatenate([[0], np.cumsum(sizes)])
    seen_tiles = []

    def tab_pred(tab):
        seen_tiles.clear()
        if not (tab[njobs:] == -1).all():
            return "a row at or above the job count holds something else than -1"
        count = np.zeros(int(seg[-1]), np.int64)
        graph_of = np.repeat(np.arange(len(sizes)), sizes)
        tiles = 0
        for j in range(njobs):
            row = tab[j]
            n = int((row >= 0).sum())
            if n == 0 or not (row[:n] >= 0).all() or not (row[n:] == -1).all() or row[:n].max() >= len(count):
                return f"job {j} is empty, has a hole or names a row outside the batch"
            np.add.at(count, row[:n], 1)
            at = 0
            while at < n:
                k = graph_of[row[at]]
                if at + sizes[k] > n or not np.array_equal(row[at:at + sizes[k]], np.arange(seg[k], seg[k + 1])):
                    return f"job {j}: member graph {k} is not whole and in node order"
                at += sizes[k]
            tiles += 2 if n > 32 else 1
        if njobs and not (count == 1).all():
            return "some row of the batch is in no slot, or in two"
        seen_tiles.append(tiles)
        return None

    def hdr_pred(hdr):
        tiles = (seen_tiles or [None])[0] if mode == "device" and njobs else 0
        empty = int((sizes == 0).sum()) if (mode == "device" and njobs) else int((sizes == 0).any())
        want = [njobs, tiles, 0, int(sizes.max()), empty]
        return None if [int(v) for v in hdr[:5]] == want else f"hdr_out[0..4] = {[int(v) for v in hdr[:5]]}, expected {want}"
    return {"tab_out": E(pred=tab_pred), "hdr_out": E(pred=hdr_pred)}


@prep_cases_of("gnnmp_chain_jobs_export")
def _(ctx):
    # the member sizes of the pair kernel's cases: cap_rows equal to the number of jobs and larger; a batch that gets no jobs at all
    shapes = ((CHAIN_PAIR_SIZES[4], "host", 0, {"align", "side"}), (CHAIN_PAIR_SIZES[4], "device", 0, {"align"}), (CHAIN_PAIR_SIZES[4], "host", 3, ()),
              (CHAIN_PAIR_SIZES[4], "device", 3, ()), (CHAIN_PAIR_SIZES[2], "device", 7, ()), ([0, 20, 0, 0, 30, 14, 0], "host", 2, ()),
              ([70, 1, 33], "device", 2, ()))
    for sizes, mode, more, tags in shapes:
        seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        njobs = bfd_jobs(sizes) if (max(sizes) <= 64 and min(sizes) > 0) else 0
        cap = njobs + more
        yield mk("gnnmp_chain_jobs_export", f"{'-'.join(map(str, sizes))}_{mode}_cap{cap}", tags,
                 [Jobs(mode, seg), Arr("tab_out", "out", shape=(cap, 64), dtype=np.int32), cap, Arr("hdr_out", "out", shape=(32,), dtype=np.int32), STREAM],
                 lambda host, v=(sizes, njobs, mode): _job_table_ref(*v))


# ------------------------------------------------------------------------------------------------------------------------------------
# variants: TABLE[export](ctx) builds the cases of ctx.variant
# ------------------------------------------------------------------------------------------------------------------------------------
def _of_variant(build):
    def cases(ctx):
        prev = _VARIANT[0]
        _VARIANT[0] = getattr(ctx, "variant", 0)
        try:
            return list(build(ctx))          # the builders are generators: every draw happens here, under the ctx's variant
        finally:
            _VARIANT[0] = prev
    return cases


TABLE = {export: _of_variant(build) for export, build in TABLE.items()}
PREP_TABLE = {export: _of_variant(build) for export, build in PREP_TABLE.items()}


# ------------------------------------------------------------------------------------------------------------------------------------
# the no-sync, no-alloc rule (include/gnnmp.h, Conventions): which exports of the table may be recorded into a HIP graph
# ------------------------------------------------------------------------------------------------------------------------------------
# An export of TABLE is CAPTURABLE — it only launches on the stream it is given — unless it is named here with the words of its own
# comment in include/gnnmp.h (or of its paragraph in the section comment that governs it) that say it waits for the stream or allocates.
# tests/test_abi_graph_capture.py checks the quotes against the header and captures, replays and re-feeds every other export.
SYNCHRONISES = {
    "gnnmp_batch_coo": "Synchronises the stream (graph prep: the two totals are read on the host)",
    "gnnmp_sort_edge_index": "Synchronises the stream (graph prep)",
    "gnnmp_unique_append": "Synchronises the stream",
    "gnnmp_induced_subgraph": "Synchronises the stream (the count is read on the host)",
    "gnnmp_rand_edge_split": "Synchronisations: 1 (the permutation's sort) + 1 when bidirected",
    "gnnmp_coalesce_edges": "Synchronises the stream (graph prep)",
    "gnnmp_compact_edges": "Synchronises the stream (graph prep)",
    "gnnmp_random_walk_pe_f32": "Synchronises the stream (graph prep)",
}
ALLOCATES = {}
WAITS_OR_ALLOCATES = re.compile(r"synchronis|hipMalloc|allocat", re.I)


def capturable():
    return sorted(e for e in TABLE if e not in SYNCHRONISES and e not in ALLOCATES)


def _squash(text):
    return " ".join(text.replace("*", " ").split())


def header_comments_of(export, path=HEADER):
    """the comment text of the RAW header that speaks for one export, whitespace-normalised: the comments that stand directly in front of
    its declaration, and — from the section comment (the one ruled off with dashes) that governs it — the paragraph headed by the
    export's name, or the whole section comment if it has no paragraph per export"""
    text = open(path).read()
    code = re.sub(r"/\*.*?\*/", lambda c: " " * len(c.group(0)), text, flags=re.S)          # same offsets, comments blanked
    m = re.search(r"\b%s\s*\(" % re.escape(export), code)
    assert m, f"{export} is not declared in the header"
    comments = [c for c in re.finditer(r"/\*.*?\*/", text, flags=re.S) if c.end() <= m.start()]
    own, end = [], code.rfind(";", 0, m.start()) + 1          # back to the end of the previous declaration
    for c in reversed(comments):
        if c.start() < end or "-----" in c.group(0):
            break
        own.append(c.group(0)[2:-2])
    out = [_squash(t) for t in own]
    section = next((c.group(0)[2:-2] for c in reversed(comments) if "-----" in c.group(0)), None)
    if section is not None:
        heads = list(re.finditer(r"^ \*   (gnnmp_\w+)\b", section, flags=re.M))
        mine = [k for k, h in enumerate(heads) if h.group(1) == export]
        if mine:
            k = mine[0]
            stop = heads[k + 1].start() if k + 1 < len(heads) else section.find("-----", heads[k].start())
            out.append(_squash(section[heads[k].start():stop if stop > 0 else len(section)]))
        elif not heads:
            out.append(_squash(section))
    return out
