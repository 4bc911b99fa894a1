"""Shapes and the plain reference of tests/test_fof.py (host side only: numpy and plain Python, no scipy).

The rule of cstone_hip_friends_of_friends: i and j of the target range are linked iff the walk of either reports the
other at h = T(0.5) * T(b).  That is the brute force wherever the walk prunes no pair within b (a pair within rounding of
b across a cell face can be pruned by the node test from one side: tests/face_support.py, tests/test_face_pairs.py);
the shapes here assert that they are of that kind (test_brute_force_is_symmetric_and_equals_the_oracles_walk).

The reference: the brute force of tests/neighbors_support.py (Case.pair_table: all pairs in the coordinate type,
d2 = dx*dx + dy*dy + dz*dz left to right, products not fused, the walk's periodic fold, strict <) at h = T(0.5) * T(b),
restricted to the target range, followed by a plain sequential union-find that labels every particle with the lowest
index of its component.  Every shape is built once per session and its reference is shared and never modified."""
import numpy as np

from helpers import Box, random_cloud, real_dtype
from neighbors_support import ANISO, Case

SENT = np.uint32(0xFFFFFFFF)  # what the tests fill the outputs with before a call


class Shape:
    def __init__(self, case, b, first=0, last=None, **info):
        self.case, self.b, self.first, self.last = case, float(b), first, case.n if last is None else last
        self.info = info  # what a premise needs to know about how the shape was built


def half_length(T, b):
    """hi = T(0.5) * T(b), as cstone_hip_friends_of_friends computes it"""
    return T(0.5) * T(b)


def make_case(oracle, x, y, z, b, box, bucket):
    T = x.dtype.type
    return Case(oracle, x, y, z, np.full(x.size, half_length(T, b), dtype=T), box, bucket)


def links(case, first, last):
    """link[i, j] over the whole cloud: i and j are both targets and j is a neighbour of i at h = b / 2 (brute force)"""
    nb = case.pair_table().copy()
    nb[:first] = False
    nb[last:] = False
    nb[:, :first] = False
    nb[:, last:] = False
    return nb


def min_labels(first, last, edges):
    """plain union-find over (a, b) index pairs of [first, last): labels[k] = lowest index of the component of first + k"""
    parent = list(range(last - first))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for a, b in edges:
        ra, rb = find(a - first), find(b - first)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(v) + first for v in range(last - first)], dtype=np.uint32)


def labels_of(link, first, last):
    a, b = np.nonzero(np.triu(link))
    return min_labels(first, last, zip(a.tolist(), b.tolist()))


def sizes_of(labels, first):
    return np.bincount(labels - first, minlength=labels.size).astype(np.uint32)[labels - first]


def catalog_of(labels, first, min_members):
    """(group_offsets, members) of the groups with at least max(min_members, 1) members by ascending label, members
    ascending"""
    order = np.argsort(labels, kind="stable")
    heads = np.flatnonzero(np.concatenate([[True], labels[order][1:] != labels[order][:-1]]))
    ends = np.concatenate([heads[1:], [labels.size]])
    keep = (ends - heads) >= max(min_members, 1)
    members = [order[a:b] + first for a, b in zip(heads[keep], ends[keep])]
    offsets = np.concatenate([[0], np.cumsum([m.size for m in members])]).astype(np.uint32)
    return offsets, (np.concatenate(members) if members else np.zeros(0, dtype=np.int64)).astype(np.uint32)


class Reference:
    def __init__(self, shape):
        s = shape
        self.link = links(s.case, s.first, s.last)
        self.labels = labels_of(self.link, s.first, s.last)
        self.sizes = sizes_of(self.labels, s.first)
        self.num_groups = int((self.labels == np.arange(s.first, s.last)).sum())
        for a in (self.link, self.labels, self.sizes):
            a.flags.writeable = False


def stub_case(x, y, z, b, box):
    """what Case.pair_table needs, for arrays that are in their final order already (a synced domain's)"""
    c = Case.__new__(Case)
    T = x.dtype.type
    c.x, c.y, c.z, c.n, c.box = x, y, z, x.size, box
    c.h = np.full(x.size, half_length(T, b), dtype=T)
    c._pairs, c._nodes = None, {}
    return c


# ---- the clouds ------------------------------------------------------------------------------------------------------

UNIT = [0, 1, 0, 1, 0, 1]
N_UNIFORM, N_CHAIN, CHAIN_GAP = 4000, 3000, 1234
BLOB_CENTERS = [(cx, cy, cz) for cx in (0.25, 0.75) for cy in (0.25, 0.75) for cz in (0.25, 0.75)]


def _cols(p, T):
    return [np.ascontiguousarray(p[:, d]).astype(T) for d in range(3)]


def blob_cloud(T, per_blob=400, sigma=0.01, seed=11):
    rng = np.random.default_rng(seed)
    p = np.concatenate([np.array(c) + rng.normal(0, sigma, (per_blob, 3)) for c in BLOB_CENTERS])
    return _cols(np.clip(p, 0, 1), T)


def corner_cloud(T, lim, n_blob=1500, n_back=300, sigma=0.03, seed=12):
    """a Gaussian blob centred on the low corner of the box, wrapped into it, and a thin uniform background"""
    rng = np.random.default_rng(seed)
    lo, ln = np.array(lim[0::2]), np.array(lim[1::2]) - np.array(lim[0::2])
    blob = lo + np.mod(rng.normal(0, sigma, (n_blob, 3)), ln)
    back = lo + rng.uniform(0, 1, (n_back, 3)) * ln
    x, y, z = _cols(np.concatenate([blob, back]), T)
    limT = np.array(lim).astype(T)
    return [np.clip(a, limT[2 * d], limT[2 * d + 1]) for d, a in enumerate((x, y, z))]


NAMES = (["n1", "n2-exact", "n2-inside", "oneleaf65", "chain", "uniform-0.5", "uniform-0.9", "uniform-1.3", "blobs",
          "corner-111", "corner-100", "corner-aniso", "clump300", "range-out", "range-in", "dense", "nolink"])

_shapes, _refs = {}, {}


def shape(oracle, name, rb):
    if (name, rb) not in _shapes:
        _shapes[name, rb] = _build(oracle, name, rb)
    return _shapes[name, rb]


def reference(oracle, name, rb):
    if (name, rb) not in _refs:
        _refs[name, rb] = Reference(shape(oracle, name, rb))
    return _refs[name, rb]


def _build(oracle, name, rb):
    T = real_dtype(rb)
    kind = name.split("-")[0]
    if kind == "n1":
        return Shape(make_case(oracle, *_cols(np.array([[0.5, 0.25, 0.75]]), T), 0.25, Box(UNIT), 16), 0.25)
    if kind == "n2":
        # the second particle at distance exactly b = 0.25 (d2 == 4 hi hi == 0.0625, all exact in T), or one ulp nearer
        x1 = T(0.25) if name == "n2-exact" else np.nextafter(T(0.25), T(0))
        p = np.array([[0, 0, 0], [x1, 0, 0]], dtype=T)
        return Shape(make_case(oracle, *_cols(p, T), 0.25, Box(UNIT), 16), 0.25)
    if kind == "oneleaf65":
        x, y, z = random_cloud(65, Box(UNIT), rb, 3, "uniform")
        return Shape(make_case(oracle, x, y, z, 0.2, Box(UNIT), 66), 0.2)
    if kind == "chain":
        # N_CHAIN points on the space diagonal, 0.9 b apart, 1.1 b between points CHAIN_GAP - 1 and CHAIN_GAP; shuffled
        b = 0.95 * np.sqrt(3.0) / (0.9 * N_CHAIN)
        steps = np.full(N_CHAIN, 0.9 * b)
        steps[0], steps[CHAIN_GAP] = 0.0, 1.1 * b
        t = 0.01 + np.cumsum(steps) / np.sqrt(3.0)
        t = t[np.random.default_rng(4).permutation(N_CHAIN)]
        p = np.stack([t, t, t], axis=1)
        return Shape(make_case(oracle, *_cols(p, T), b, Box(UNIT), 16), b)
    if kind == "uniform":
        b = float(name.split("-")[1]) * N_UNIFORM ** (-1.0 / 3.0)
        x, y, z = random_cloud(N_UNIFORM, Box(UNIT), rb, 7, "uniform")
        return Shape(make_case(oracle, x, y, z, b, Box(UNIT, (1, 1, 1)), 16), b)
    if kind == "blobs":
        return Shape(make_case(oracle, *blob_cloud(T), 0.008, Box(UNIT), 64), 0.008)
    if kind == "corner":
        lim, bc = (ANISO, (1, 1, 1)) if name == "corner-aniso" else (UNIT, tuple(int(c) for c in name.split("-")[1]))
        return Shape(make_case(oracle, *corner_cloud(T, lim), 0.015, Box(lim, bc), 32), 0.015)
    if kind == "clump300":
        x, y, z = random_cloud(2000, Box(UNIT), rb, 9, "uniform")
        for a in (x, y, z):
            a[-300:] = a[0]  # a leaf that cannot be split
        return Shape(make_case(oracle, x, y, z, 0.05, Box(UNIT, (1, 1, 1)), 64), 0.05)
    if kind == "range":
        return _build_range(oracle, name, T)
    if kind == "dense":
        x, y, z = random_cloud(1200, Box(UNIT), rb, 13, "uniform")
        return Shape(make_case(oracle, x, y, z, 0.3, Box(UNIT), 16), 0.3)
    if kind == "nolink":
        x, y, z = random_cloud(1500, Box(UNIT), rb, 14, "uniform")
        probe = stub_case(x, y, z, 1.0, Box(UNIT))
        d2 = sum((a[None, :] - a[:, None]) ** 2 for a in (probe.x, probe.y, probe.z))
        np.fill_diagonal(d2, np.inf)
        b = 0.9 * float(np.sqrt(d2.min()))
        return Shape(make_case(oracle, x, y, z, b, Box(UNIT, (1, 1, 1)), 16), b, dmin=float(np.sqrt(d2.min())))
    raise ValueError(name)


def _build_range(oracle, name, T):
    """n = 600: two clumps of 40, 0.9 b away from a bridge particle and 1.27 b from each other, over a background that
    keeps more than b away from all of them.  In SFC order the bridge lies in front of both clumps: a range that starts
    behind it leaves it out, one that starts at it takes it in.  Neither end of the range is a multiple of 64."""
    b = 0.05
    rng = np.random.default_rng(21)
    bridge = np.array([0.1, 0.1, 0.1])
    ca, cb = bridge + [0.9 * b, 0, 0], bridge + [0, 0.9 * b, 0]
    clump = lambda c: c + rng.uniform(-0.002, 0.002, (40, 3))  # noqa: E731
    near = np.array([[0.01, 0.01, 0.01], [0.02, 0.01, 0.01], [0.01, 0.02, 0.02]])  # in front of the bridge, > b away
    back = rng.uniform(0.3, 1.0, (600 - 81 - len(near), 3))
    p = np.concatenate([bridge[None, :], clump(ca), clump(cb), near, back])
    x, y, z = _cols(p, T)
    case = make_case(oracle, x, y, z, b, Box(UNIT), 16)
    where = lambda q: np.flatnonzero((case.x == q[0]) & (case.y == q[1]) & (case.z == q[2]))  # noqa: E731
    pb = int(where((x[0], y[0], z[0]))[0])
    ia = np.concatenate([where((x[k], y[k], z[k])) for k in range(1, 41)])
    ib = np.concatenate([where((x[k], y[k], z[k])) for k in range(41, 81)])
    first = pb + 1 if name == "range-out" else pb
    return Shape(case, b, first, 531, bridge=pb, clump_a=ia, clump_b=ib)
