"""Clouds and the numpy restatement for tests/test_fof_mr.py and tests/fof_mr_worker.py (host side only).

The restatement of friends-of-friends across ranks works on what every rank holds after a sync -- its arrays with the
halos, and for every entry the particle's global id, i.e. its position in the global SFC order: local components by the
brute force of tests/fof_support.py over EVERYTHING present on the rank, then rounds of lower / exchange until no rank
changes an assigned label.  The brute force is what the ranks' walks give wherever no pair within b is pruned by a node
test from both sides (tests/fof_support.py); the cloud "faces" puts that to the test across a rank boundary."""
import numpy as np

import fof_support as fs

N_UNIFORM = 6000
SERPENTINE_B, SERPENTINE_RUNS = 0.01, 32


def uniform_cloud(T):
    """6 000 uniform particles in the unit box, b = 0.9 x the mean separation"""
    x, y, z = np.random.default_rng(101).uniform(0, 1, (3, N_UNIFORM))
    return [a.astype(T) for a in (x, y, z)], 0.9 * N_UNIFORM ** (-1.0 / 3.0)


def serpentine_cloud(runs=SERPENTINE_RUNS, b=SERPENTINE_B):
    """ONE chain at a spacing of at most 0.8 b: `runs` runs along x from 0.05 to 0.95 at y = 0.05 + 0.9 r / (runs - 1),
    z = 0.37, joined at alternating ends by points along y.  Neighbouring runs are about 3 b apart: one group, and the
    only way from one run to the next is through its far end"""
    per_run = int(np.ceil(0.9 / (0.8 * b))) + 1
    xs = np.linspace(0.05, 0.95, per_run)
    ys = 0.05 + 0.9 * np.arange(runs) / (runs - 1)
    px, py = [], []
    for r in range(runs):
        px.append(xs if r % 2 == 0 else xs[::-1])
        py.append(np.full(per_run, ys[r]))
        if r + 1 < runs:
            seg = int(np.ceil((ys[r + 1] - ys[r]) / (0.8 * b)))
            px.append(np.full(seg - 1, px[-1][-1]))
            py.append(np.linspace(ys[r], ys[r + 1], seg + 1)[1:-1])
    x, y = np.concatenate(px), np.concatenate(py)
    return [x, y, np.full(x.size, 0.37)], b


CLOUDS = {  # name: (coordinate type, boundary conditions)
    "uniform-open": (np.float64, (0, 0, 0)),
    "uniform-pbc": (np.float64, (1, 1, 1)),
    "uniform-pbc-f32": (np.float32, (1, 1, 1)),
    "serpentine": (np.float64, (1, 1, 1)),  # (periodic: the box stays the unit cube although z is constant)
}


FACES_N, FACES_SHIFT = 1200, 0.1


def faces_cloud():
    """600 pairs across the x faces of the level-3 cells of the anisotropic open box (tests/face_support.py), every pair
    0.1 cell edges apart up to the rounding of its coordinates, and b = twice the median of the pairs' threshold h: about
    half of the pairs are linked, every one of them within a few ulp of b, and hardly any particle has a third one
    within b -- a group IS its pair's own link.  Particles 2p and 2p + 1 are a pair; the last two particles sit in two
    opposite corners of the box, so that the limits fitted to an open domain are the box's and the faces stay faces"""
    import face_support as fa
    from helpers import Box

    x, y, z, _, _ = fa.face_cloud(np.float64, fa.ANISO, (0, 0, 0), axis_mix=False, n=FACES_N, edge_every=0,
                                  shift=(FACES_SHIFT, FACES_SHIFT))
    x, y, z = [np.concatenate([a, fa.ANISO[2 * d:2 * d + 2]]) for d, a in enumerate((x, y, z))]
    even = np.arange(0, FACES_N, 2)
    h = fa.threshold_h(fs.stub_case(x, y, z, 1.0, Box(fa.ANISO, (0, 0, 0))), even, even + 1)
    return [x, y, z], 2.0 * float(np.sort(h)[h.size // 2])


def cloud_limits(name):
    """the box a domain is made with for the cloud"""
    import face_support as fa

    return list(map(float, fa.ANISO)) if name == "faces" else [0.0, 1.0] * 3


def cloud(name):
    """((x, y, z), b, bc).  "faces" is not among CLOUDS: it runs on two ranks only (tests/test_face_pairs.py)"""
    if name == "faces":
        coords, b = faces_cloud()
        return coords, b, (0, 0, 0)
    T, bc = CLOUDS[name]
    (x, y, z), b = serpentine_cloud() if name == "serpentine" else uniform_cloud(T)
    return (x, y, z), b, bc


def groups_of(x, y, z, b, box):
    """(labels, sizes, number of groups) of the brute force over arrays in their final order: labels[k] = lowest index"""
    case = fs.stub_case(x, y, z, b, box)
    labels = fs.labels_of(fs.links(case, 0, case.n), 0, case.n)
    return labels, fs.sizes_of(labels, 0), int((labels == np.arange(case.n)).sum())


class RankPart:
    """what one rank holds: coordinates with halos, the global id of every entry, the assigned range"""

    def __init__(self, x, y, z, ids, start, end):
        self.x, self.y, self.z, self.ids, self.start, self.end = x, y, z, np.asarray(ids, dtype=np.uint64), start, end


def model_rounds(parts, b, box, max_rounds=100000):
    """(labels per rank, rounds): the rounds of cstone_hip_domain_mr_fof restated.  A round lowers every label to the
    minimum of its local component, then the halos take their owners' labels; the first round in which no rank lowered
    an assigned label is the last"""
    total = sum(p.end - p.start for p in parts)
    comps, labels = [], []
    for p in parts:
        comps.append(groups_of(p.x, p.y, p.z, b, box)[0].astype(np.int64) if p.ids.size else np.zeros(0, dtype=np.int64))
        labels.append(p.ids.copy())  # a halo's id is its owner's
    rounds = 0
    while rounds < max_rounds:
        rounds += 1
        changed = False
        owners = np.zeros(total, dtype=np.uint64)
        for p, comp, lab in zip(parts, comps, labels):
            low = np.full(lab.size, np.iinfo(np.uint64).max, dtype=np.uint64)
            np.minimum.at(low, comp, lab)
            new = low[comp] if lab.size else lab
            changed = changed or bool((new[p.start:p.end] < lab[p.start:p.end]).any())
            lab[:] = new
            owners[p.ids[p.start:p.end].astype(np.int64)] = lab[p.start:p.end]
        for p, lab in zip(parts, labels):
            halo = np.ones(lab.size, dtype=bool)
            halo[p.start:p.end] = False
            lab[halo] = owners[p.ids[halo].astype(np.int64)]
        if not changed:
            break
    return labels, rounds
