"""The restatement and the shapes of tests/test_adapt_h.py (host side only, numpy and the CPU oracle).

* adapt: the rule of cstone_hip_adapt_smoothing_lengths (include/cstone_hip.h) for all targets of [first, last) at once,
  in the coordinate type: every operation is one numpy ufunc on arrays of that type (numpy fuses nothing), min and max
  are written as the comparisons the header names.  The count of one iteration is oracle.find_neighbors(ngmax = 1) with
  the current h vector: the walk tests/test_neighbors.py proves equal to the kernel's and to the brute force.
* brute_counts: the brute force of neighbors_support.pair_table for given rows and a given h.
* shape(name, rb): the clouds with their parameters, built once per session; result(name, rb): their restated results,
  computed once and shared by every test."""
import collections

import numpy as np

import neighbors_support as ns
from helpers import Box, random_cloud, real_dtype

NOT_CONVERGED, CAPPED, STALLED, WALKS = 0x100, 0x200, 0x400, 0xFF
FLAGS = NOT_CONVERGED | CAPPED | STALLED
INF = float("inf")

Params = collections.namedtuple("Params", "ng0 tol max_iter grow_limit")
Result = collections.namedtuple("Result", "h counts status trace")

_oracle_obj = None


def the_oracle():
    global _oracle_obj
    if _oracle_obj is None:
        import os

        from oracle import oracle as orc

        if not os.path.exists(orc.Oracle.libpath):
            orc.build("liboracle")
        _oracle_obj = orc.Oracle()
    return _oracle_obj


def oracle_counts(case, h, first, last):
    """counts of the oracle's walk for the h vector `h` (all particles), targets [first, last)"""
    return the_oracle().find_neighbors(case.x, case.y, case.z, h, first, last, case.box, case.o, case.layout, case.cen,
                                       case.siz, 1, 1.0)[1].astype(np.int64)


def adapt(case, first, last, params, h0=None):
    """Result(h: the whole vector after the call, counts [last - first], status [last - first] as the kernel packs it,
    trace: per walk (h of the targets, active mask, counts) as they were when the walk was made)"""
    T = case.x.dtype.type
    ng0, tol, max_iter = int(params.ng0), int(params.tol), int(params.max_iter)
    n = last - first
    h = (case.h if h0 is None else h0).astype(T).copy()
    hw = h[first:last].copy()
    inf = T(INF)
    lo, hi = np.zeros(n, dtype=T), np.full(n, inf, dtype=T)
    with np.errstate(all="ignore"):
        hcap = hw * T(np.float32(params.grow_limit))
    nn, walks = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    flags = np.zeros(n, dtype=np.uint32)
    active = np.ones(n, dtype=bool)
    trace, it = [], 0
    while active.any():
        h[first:last] = hw
        cnt = oracle_counts(case, h, first, last)
        trace.append((hw.copy(), active.copy(), cnt.copy()))
        nn = np.where(active, cnt, nn)
        walks += active
        converged = (nn + tol >= ng0) & (nn <= ng0 + tol)
        a = active & ~converged
        if it == max_iter:
            flags[a] |= NOT_CONVERGED
            break
        low = nn + tol < ng0
        lo = np.where(a & low, hw, lo)
        hi = np.where(a & ~low, hw, hi)
        capped = a & low & (hw >= hcap)
        flags[capped] |= CAPPED
        a = a & ~capped
        with np.errstate(all="ignore"):
            q = T(ng0) / np.maximum(nn, 1).astype(T)
            q = np.where(q < T(0.125), T(0.125), q)
            q = np.where(q > T(8), T(8), q)
            t = (T(2) + q) / T(3)
            t = (T(2) * t + q / (t * t)) / T(3)
            hp = hw * t
            hp = np.where(hcap < hp, hcap, hp)
            bisect = (hi < inf) & ~((lo < hp) & (hp < hi))
            hp = np.where(bisect, T(0.5) * (lo + hi), hp)
        assert q.dtype == t.dtype == hp.dtype == hw.dtype == np.dtype(T)
        stalled = a & (hp == hw)
        flags[stalled] |= STALLED
        a = a & ~stalled
        hw = np.where(a, hp, hw)
        active = a
        it += 1
    h[first:last] = hw
    status = (np.minimum(walks, 255).astype(np.uint32) | flags).astype(np.uint32)
    return Result(h, nn.astype(np.uint32), status, trace)


def brute_counts(case, rows, h_rows):
    """number of j != i with |r_j - r_i|^2 < 4 h_i^2 for the targets `rows` with smoothing lengths h_rows, evaluated as
    neighbors_support.Case.pair_table does: in the coordinate type, left to right, folded by dx - len * rint(dx * inv)
    on periodic axes when the target's +-2h cube leaves the box"""
    T = case.x.dtype.type
    rows = np.asarray(rows, dtype=np.int64)
    if rows.size == 0:
        return np.zeros(0, dtype=np.int64)
    lim = case.box.lim.astype(T)
    lo, hi = lim[0::2], lim[1::2]
    ln = hi - lo
    inv = T(1) / ln
    P = (case.x, case.y, case.z)
    s = T(2) * h_rows
    inside = np.ones(rows.size, dtype=bool)
    for d in range(3):
        inside &= (P[d][rows] - s >= lo[d]) & (P[d][rows] + s <= hi[d])
    periodic = [int(b) == 1 for b in case.box.bc]
    use = (~inside) & any(periodic)
    d2 = None
    for d in range(3):
        dx = P[d][None, :] - P[d][rows, None]
        if periodic[d]:
            dx = np.where(use[:, None], dx - ln[d] * np.rint(dx * inv[d]), dx)
        sq = dx * dx
        d2 = sq if d2 is None else d2 + sq
    assert d2.dtype == case.x.dtype
    nb = d2 < (T(4) * h_rows * h_rows)[:, None]
    nb[np.arange(rows.size), rows] = False
    return nb.sum(1).astype(np.int64)


def cube_inside(case, rows, h_rows):
    """the insideBox test of the walk for the targets `rows` at h_rows"""
    T = case.x.dtype.type
    lim = case.box.lim.astype(T)
    s = T(2) * h_rows
    inside = np.ones(len(rows), dtype=bool)
    for d, p in enumerate((case.x, case.y, case.z)):
        inside &= (p[rows] - s >= lim[2 * d]) & (p[rows] + s <= lim[2 * d + 1])
    return inside


def sfc_order(oracle, x, y, z, box, curve=ns.HILBERT, kb=64):
    """the permutation neighbors_support.Case applies to its input arrays"""
    keys = oracle.compute_sfc_keys(curve, kb, x, y, z, box)
    return oracle.sort_pairs(keys, np.arange(x.size))[1]


def knn_h(x, y, z, k):
    """per particle the h at which an open box gives exactly k neighbours: 2 h halfway between the distances to the k-th
    and the (k + 1)-th nearest other particle (float64)"""
    X = np.stack([a.astype(np.float64) for a in (x, y, z)], 1)
    out = np.empty(X.shape[0])
    for a in range(0, X.shape[0], 500):
        d = np.sqrt(((X[a:a + 500, None, :] - X[None, :, :]) ** 2).sum(2))
        d.partition((k, k + 1), axis=1)  # column 0 is the particle itself
        out[a:a + 500] = 0.25 * (d[:, k] + d[:, k + 1])
    return out


# ---- the shapes ------------------------------------------------------------------------------------------------------

class Shape:
    def __init__(self, case, first, last, params):
        self.case, self.first, self.last, self.params = case, first, last, params


N_CLOUD = 3000
STD = Params(50, 5, 10, 2.0)  # the parameters of the convergence statement

_shapes, _results = {}, {}


def shape(name, rb):
    if (name, rb) not in _shapes:
        _shapes[name, rb] = _build(name, rb)
    return _shapes[name, rb]


def result(name, rb):
    """the restated result of the shape, computed once"""
    if (name, rb) not in _results:
        s = shape(name, rb)
        _results[name, rb] = adapt(s.case, s.first, s.last, s.params)
    return _results[name, rb]


def cloud_case(kind, rb, n=N_CLOUD, ng0=50, seed=11, bucket=64, exact=None):
    """n particles in the open unit box, uniform or in six Gaussian clumps (helpers.random_cloud), with h0 = the h of
    exactly ng0 neighbours times U(0.6, 1.4); exact = (a, b): the particles a .. b - 1 in SFC order keep factor 1"""
    oracle = the_oracle()
    T = real_dtype(rb)
    box = Box([0, 1])
    x, y, z = random_cloud(n, box, rb, seed, kind)
    order = sfc_order(oracle, x, y, z, box)
    factor = np.random.default_rng(seed + 1).uniform(0.6, 1.4, n)
    if exact is not None:
        factor[exact[0]:exact[1]] = 1.0
    h = np.empty(n, dtype=T)
    h[order] = (knn_h(x[order], y[order], z[order], ng0) * factor).astype(T)
    return ns.Case(oracle, x, y, z, h, box, bucket)


def mixed_cloud_case(rb):
    """clumps and void in the same waves: 2 400 particles in six clumps and 600 spread over the box, h0 as in cloud_case
    with the waves 8 .. 11 (particles 512 .. 767 in SFC order) exact"""
    oracle = the_oracle()
    T = real_dtype(rb)
    box = Box([0, 1])
    cl = random_cloud(2400, box, rb, 21, "clustered")
    un = random_cloud(600, box, rb, 22, "uniform")
    x, y, z = [np.concatenate(p) for p in zip(cl, un)]
    order = sfc_order(oracle, x, y, z, box)
    factor = np.random.default_rng(23).uniform(0.6, 1.4, x.size)
    factor[512:768] = 1.0
    h = np.empty(x.size, dtype=T)
    h[order] = (knn_h(x[order], y[order], z[order], 50) * factor).astype(T)
    return ns.Case(oracle, x, y, z, h, box, 64)


def _build(name, rb):
    oracle = the_oracle()
    kind = name.split("-")[0]
    if kind in ("uniform", "clumps"):
        case = cloud_case("uniform" if kind == "uniform" else "clustered", rb)
        return Shape(case, 0, case.n, STD)
    if kind == "uneven":
        case = mixed_cloud_case(rb)
        return Shape(case, 0, case.n, Params(50, 5, 10, INF))
    if kind == "tiny":  # tiny-n1, tiny-n2, tiny-n65: one leaf
        n = int(name.split("-")[1][1:])
        case = ns.spec(oracle, f"single-n{n}-open", rb).case
        p = {1: Params(5, 0, 3, INF), 2: Params(2, 1, 10, INF), 65: Params(20, 2, 10, INF)}[n]
        return Shape(case, 0, n, p)
    if kind == "range":  # range-<count>: targets 37 .. 37 + count - 1 of 600
        case = cloud_case("uniform", rb, n=600, ng0=30, seed=31, bucket=16)
        cnt = int(name.split("-")[1])
        return Shape(case, 37, 37 + cnt, Params(30, 3, 10, 2.0))
    if kind == "fold":  # fold-111, fold-102: the anisotropic box, periodic and mixed faces
        s = ns.spec(oracle, f"aniso-{name.split('-')[1]}-b16", rb)
        f, l = s.ranges[0]
        return Shape(s.case, f, l, Params(12, 2, 10, INF))
    if kind == "long":  # long-clustered-b200, long-clump300: leaves of more than 64 and 128 particles
        s = ns.spec(oracle, name[len("long-"):], rb)
        f, l = s.ranges[0]
        return Shape(s.case, f, l, Params(40, 4, 10, 4.0))
    if kind == "edge":
        case = cloud_case("uniform", rb, n=600, ng0=30, seed=31, bucket=16)
        what = name.split("-")[1]
        p = {"tol0": Params(30, 0, 10, 2.0), "toomany": Params(700, 3, 6, INF), "toomanycapped": Params(700, 3, 10, 3.0),
             "grow1": Params(30, 3, 10, 1.0), "growinf": Params(30, 3, 10, INF), "iter0": Params(30, 3, 0, 2.0)}[what]
        return Shape(case, 37, 600 - 11, p)
    raise ValueError(name)


GPU_SHAPES = (["tiny-n1", "tiny-n2", "tiny-n65"] + [f"range-{c}" for c in (1, 63, 64, 65, 257)] +
              ["uneven", "fold-111", "fold-102", "long-clustered-b200", "long-clump300"] +
              [f"edge-{w}" for w in ("tol0", "toomany", "toomanycapped", "grow1", "growinf", "iter0")])
