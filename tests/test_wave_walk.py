"""The three users of the batched walk of csrc/wave_walk.hpp -- cstone_hip_sphere_profiles, cstone_hip_pair_counts_cross and
cstone_hip_knn -- held against each other and against the numpy brute force on the same tree.  For a centre c and a
radius r all three count the particles with d2 < r * r (offset, fold, d2 and the product in the coordinate type): the
profile with the single bin [0, r) (edges [0, 1] scaled by r), the cross pair counts of the one query c with the edges
[0, r], and the k nearest neighbours with k = 256 and rmax = r, whose radius is strict.  The kNN passes its own hooks to
the walk (a second node test before the push, the pushed children sorted by distance); a hook that made it visit less
than the plain walk of the other two would show here as a smaller count.

The radii come from the brute force alone: counts from 0 up to, but not above, 256, asserted before the device is called.
Every call ends in cstone_hip_ctx_sync (the Setup classes of the three test modules), which fails unless the context's
sticky error word is 0."""
import numpy as np
import pytest

import sphere_support as ss
import test_knn as tk
import test_pair_counts as tp
import test_sphere_profiles as tsp
from helpers import Box, random_cloud, real_dtype
from neighbors_support import Case

K = 256
UNIT = [0, 1, 0, 1, 0, 1]
BCS = {"open": (0, 0, 0), "periodic": (1, 1, 1)}
ONE_BIN = [0.0, 1.0]


def with_box(case, bc):
    """the same cloud and tree in the box with these boundaries (the keys and the node geometry do not look at them)"""
    c = Case.__new__(Case)
    c.__dict__.update(case.__dict__)
    c.box = Box(np.asarray(case.box.lim).tolist(), bc)
    return c


def radii(case, qc, targets):
    """one radius per query, in the coordinate type, from the brute force alone: just above the distance of the target-th
    nearest particle (half the distance of the nearest particle that is not at the centre for the target 0), below half a
    periodic edge, and the target halved until no more than K particles lie inside (coincident particles enter together)"""
    T = case.x.dtype.type
    d2 = ss.d2_table((case.x, case.y, case.z), qc, case.box.lim, case.box.bc)
    lim = np.asarray(case.box.lim, dtype=np.float64)
    per = [lim[2 * a + 1] - lim[2 * a] for a in range(3) if int(case.box.bc[a]) == 1]
    r = np.empty(len(targets), dtype=T)
    for q, t in enumerate(targets):
        s = np.sort(d2[q])
        while True:
            base = s[min(t, s.size) - 1] if t else T(0)  # (0 also at a clump: the radius must stay above 0)
            rq = np.nextafter(np.sqrt(base), T(np.inf)) if base > 0 else T(0.5) * np.sqrt(s[s > 0][0])
            if per:
                rq = min(rq, T(0.49 * min(per)))
            if t == 0 or int((d2[q] < rq * rq).sum()) <= K:
                break
            t //= 2
        r[q] = rq
    assert r.dtype == case.x.dtype and (r > 0).all()
    return r


def points(case, num_at_particles, num_random, seed):
    rng = np.random.default_rng(seed)
    at = rng.choice(case.n, num_at_particles, replace=False)
    a = np.stack([case.x[at], case.y[at], case.z[at]], axis=1).astype(np.float64)
    return np.concatenate([a, rng.uniform(0.02, 0.98, (num_random, 3))])


def spread(lo, hi, num):
    return np.linspace(lo, hi, num).round().astype(int).tolist()


def check(hip, case, qc, r, top):
    """the three calls and the brute force on (qc[q], r[q]); top: what the largest brute-force count must reach"""
    T = case.x.dtype.type
    qc = np.asarray(qc, dtype=T)
    Q = qc.shape[0]
    knn, sphere, pair = tk.Setup(hip, case), tsp.Setup(hip, case, None), tp.Setup(hip, case)
    ref = knn.reference(qc, K, r)  # the brute force: ids ordered by (d2, index), their d2, the counts
    inside = ref.d2_table < (r * r)[:, None]
    count = inside.sum(axis=1)
    assert count.min() == 0 and top <= count.max() <= K, (count.min(), count.max())
    assert np.array_equal(ref.counts, count)

    got_s = sphere.call(qc, r, ONE_BIN)
    tsp.agree(got_s, sphere.reference(qc, r, ONE_BIN), with_sums=False)
    got_k = knn.call(qc, K, rmax=r)
    tk.agree(got_k, ref)
    of_sphere = got_s["counts"][:Q, 0].tolist()
    of_knn = got_k["counts"][:Q].view(np.uint32).tolist()
    of_pair = []
    for q in range(Q):
        got_p = pair.cross(qc[q], [0.0, float(r[q])], stats=True)
        tp.untouched(got_p, start=1)
        tp.untouched(got_p, keys=("sums",))
        assert got_p["stats"][1] == int(got_p["counts"][0]) <= got_p["stats"][0]
        of_pair.append(int(got_p["counts"][0]))
        ids = got_k["neighbors"][q, :count[q]].view(np.uint32)
        assert set(ids.tolist()) == set(np.flatnonzero(inside[q]).tolist()), q
    assert of_sphere == of_pair == of_knn == count.tolist()
    hip.sync()
    return sphere, pair


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", list(BCS))
@pytest.mark.parametrize("rb", [32, 64])
def test_hip_three_walks_on_the_deepest_tree(hip, oracle, rb, boundary):
    """the clump cloud of test_sphere_profiles.deep_setup (the deepest level, leaves of 71 and 151 coincident particles),
    Q = 65: the two clumps, 20 particles and 43 points of the box.  Then the 65 centres as the targets of ONE cross call (a
    full wave and a wave of one target) with a common radius, against the profile rows of that radius summed"""
    T = real_dtype(rb)
    s, clump_a, clump_b = tsp.deep_setup(hip, oracle, rb)
    case = with_box(s.case, BCS[boundary])
    qc = np.concatenate([[clump_a, clump_b], points(case, 20, 43, 3)]).astype(T)
    r = radii(case, qc, [100, 200] + spread(1, K, 20) + spread(0, K, 43))
    sphere, pair = check(hip, case, qc, r, K)

    common = np.full(65, np.sort(r)[32], dtype=T)
    rows = sphere.reference(qc, common, ONE_BIN).counts[:, 0]
    assert rows.sum() > 1000
    got_s = sphere.call(qc, common, ONE_BIN)
    got_p = pair.cross(qc, [0.0, float(common[0])], stats=True)
    assert np.array_equal(got_s["counts"][:65, 0].view(np.uint64), rows)
    assert int(got_p["counts"][0]) == got_p["stats"][1] == int(rows.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", list(BCS))
@pytest.mark.parametrize("rb", [32, 64])
def test_hip_three_walks_open_every_node(hip, oracle, rb, boundary):
    """200 particles in the middle of the unit box at bucket size 8; the first query, from the centre of the box with a
    radius of 0.45, holds all of them and its node test prunes no node of the tree (restated: ss.node_skip_table; the
    list of the kNN is never full, so its threshold stays at the radius, and the margin of the pair counts is the
    wider one); 11 more queries with counts from 0 to 200"""
    T = real_dtype(rb)
    x, y, z = [(T(0.3) + T(0.4) * a).astype(T) for a in random_cloud(200, Box(UNIT), rb, 37, "uniform")]
    case = Case(oracle, x, y, z, np.zeros_like(x), Box(UNIT, BCS[boundary]), 8)
    assert case.o["num_nodes"] > 64
    qc = np.concatenate([[[0.5, 0.5, 0.5]], points(case, 4, 7, 5)]).astype(T)
    r = radii(case, qc, [200] + spread(1, 200, 4) + spread(0, 200, 7))
    r[0] = T(0.45)
    assert not ss.node_skip_table(case, qc[:1], r[:1], ONE_BIN)[:, :case.o["num_nodes"]].any()
    check(hip, case, qc, r, 200)


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", list(BCS))
@pytest.mark.parametrize("rb", [32, 64])
def test_hip_three_walks_on_a_one_leaf_tree(hip, oracle, rb, boundary):
    """40 particles, bucket size 64: the root is a leaf.  The profile and the pair counts take the front of the walk, the
    kNN its seed descent alone.  Open box: up to all 40 inside; periodic: a radius of 0.49 holds half the box's volume"""
    T = real_dtype(rb)
    x, y, z = random_cloud(40, Box(UNIT), rb, 31, "uniform")
    case = Case(oracle, x, y, z, np.zeros_like(x), Box(UNIT, BCS[boundary]), 64)
    assert case.o["num_nodes"] == 1
    qc = points(case, 3, 5, 7).astype(T)
    r = radii(case, qc, spread(1, 40, 3) + spread(0, 40, 5))
    check(hip, case, qc, r, 40 if boundary == "open" else 10)
