"""Barnes-Hut gravity on the focus tree (csrc/gravity.hip): the multipole upsweep, the group walk and their entry points
(cstone_hip_upsweep_multipoles, cstone_hip_compute_gravity, cstone_hip_domain_compute_gravity, Domain::computeGravity).

The references live here: a direct sum (NumPy, float64, chunked) and a NumPy restatement of the walk (same group boxes,
same evaluateMac arithmetic in the coordinates' precision, same expansions) that also counts the interactions."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cornerstone-octree_amd", "build", "gravity_example")
MAX_LEVEL = {32: 10, 64: 21}


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def direct_sum(x, y, z, m, targets, G=1.0, eps2=0.0, chunk_elems=1 << 22):
    """(a (len(targets), 3), phi) of every source on the targets, float64, the target itself skipped"""
    x, y, z, m = [np.asarray(a, dtype=np.float64) for a in (x, y, z, m)]
    targets = np.asarray(targets, dtype=np.int64)
    acc = np.zeros((targets.size, 3))
    phi = np.zeros(targets.size)
    step = max(1, chunk_elems // x.size)
    for s in range(0, targets.size, step):
        t = targets[s:s + step]
        dx, dy, dz = x[None, :] - x[t, None], y[None, :] - y[t, None], z[None, :] - z[t, None]
        r2 = dx * dx + dy * dy + dz * dz + eps2
        r2[np.arange(t.size), t] = np.inf  # the target itself
        rinv = 1.0 / np.sqrt(r2)
        mr = m[None, :] * rinv
        mr3 = mr * rinv * rinv
        acc[s:s + step] = G * np.stack([(mr3 * dx).sum(1), (mr3 * dy).sum(1), (mr3 * dz).sum(1)], 1)
        phi[s:s + step] = -G * mr.sum(1)
    return acc, phi


def m2p(dx, dy, dz, mp, order, eps2):
    """acceleration / potential of the multipoles mp (k, 8) on the points d = r - c (t, k), summed over k"""
    r2 = dx * dx + dy * dy + dz * dz + eps2
    rinv = 1.0 / np.sqrt(r2)
    M = mp[None, :, 0]
    mr3 = M * rinv ** 3
    a = [-mr3 * dx, -mr3 * dy, -mr3 * dz]
    phi = -M * rinv
    if order == 2:
        qxx, qxy, qxz, qyy, qyz, qzz = [mp[None, :, k] for k in range(1, 7)]
        qx = qxx * dx + qxy * dy + qxz * dz
        qy = qxy * dx + qyy * dy + qyz * dz
        qz = qxz * dx + qyz * dy + qzz * dz
        dqd = dx * qx + dy * qy + dz * qz
        r5 = rinv ** 5
        f = 2.5 * dqd * r5 * rinv * rinv
        a = [a[0] + r5 * qx - f * dx, a[1] + r5 * qy - f * dy, a[2] + r5 * qz - f * dz]
        phi = phi - 0.5 * dqd * r5
    return np.stack([s.sum(1) for s in a], 1), phi.sum(1)


def walk_reference(t, lo, hi, order, G=1.0, eps2=0.0):
    """the walk of cstone_hip_compute_gravity for the target group [lo, hi) restated: (a, phi, p2p counts, m2p counts)
    per target.  A group longer than 64 is walked as the kernel does, one run of 64 targets at a time, each run with its
    own box.  t: the dict of tree_state() (or of a hand-built tree with the same keys)"""
    if hi - lo > 64:
        runs = [walk_reference(t, s, min(hi, s + 64), order, G, eps2) for s in range(lo, hi, 64)]
        return tuple(np.concatenate(parts) for parts in zip(*runs))
    rdt = t["rdt"]
    xs, ys, zs = t["x"], t["y"], t["z"]
    ctr = t["centers"]
    # the box of the targets, in the coordinates' precision
    lo3 = [a[lo:hi].min() for a in (xs, ys, zs)]
    hi3 = [a[lo:hi].max() for a in (xs, ys, zs)]
    tc = [(a + b) * rdt(0.5) for a, b in zip(lo3, hi3)]
    ts = [(b - a) * rdt(0.5) for a, b in zip(lo3, hi3)]
    # evaluateMac for every node at once, the same operations in the same precision (no contraction in NumPy)
    d = []
    for k in range(3):
        v = np.abs(tc[k] - ctr[:, k]) - ts[k]
        v = v + np.abs(v)
        d.append(v * rdt(0.5))
    R2 = d[0] * d[0] + (d[1] * d[1] + d[2] * d[2])
    opened = R2 < np.abs(ctr[:, 3])
    child, itl, layout = t["child_offsets"], t["internal_to_leaf"], t["layout"]
    m2p_nodes, p2p_leaves = [], []
    stack = [0]
    while stack:
        n = stack.pop()
        if ctr[n, 3] == 0:
            continue
        if not opened[n]:
            m2p_nodes.append(n)
        elif child[n] == 0:
            p2p_leaves.append(itl[n])
        else:
            stack.extend(range(child[n] + 7, child[n] - 1, -1))
    tg = np.arange(lo, hi)
    X = [a.astype(np.float64) for a in (xs, ys, zs)]
    acc = np.zeros((tg.size, 3))
    phi = np.zeros(tg.size)
    if m2p_nodes:
        nodes = np.array(m2p_nodes)
        c64 = ctr[nodes, :3].astype(np.float64)
        dd = [X[k][tg, None] - c64[None, :, k] for k in range(3)]
        a, p = m2p(*dd, t["multipoles"][nodes].astype(np.float64), order, eps2)
        acc += a
        phi += p
    p2p_counts = np.zeros(tg.size, dtype=np.int64)
    if p2p_leaves:
        src = np.concatenate([np.arange(layout[lf], layout[lf + 1]) for lf in p2p_leaves])
        m64 = t["m"].astype(np.float64)[src]
        dd = [X[k][None, src] - X[k][tg, None] for k in range(3)]
        r2 = dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2] + eps2
        self_ = src[None, :] == tg[:, None]
        rinv = np.where(self_, 0.0, 1.0 / np.sqrt(np.where(self_, 1.0, r2)))
        mr = m64[None, :] * rinv
        mr3 = mr * rinv * rinv
        acc += np.stack([(mr3 * dd[k]).sum(1) for k in range(3)], 1)
        phi -= mr.sum(1)
        p2p_counts = src.size - self_.sum(1)
    return G * acc, G * phi, p2p_counts, np.full(tg.size, len(m2p_nodes))


# ---------------------------------------------------------------------------------------------------------------------
# set-up
# ---------------------------------------------------------------------------------------------------------------------
def clustered_cloud(n, seed):
    rng = np.random.default_rng(seed)
    from cstone_amd.clouds import BLOB_CENTRES

    pos = np.array(BLOB_CENTRES)[rng.integers(0, 8, n)] + rng.normal(0, 1.0 / 40.0, (n, 3))
    pos = np.clip(pos, 0.0, 1.0)
    return pos[:, 0], pos[:, 1], pos[:, 2], rng.uniform(0.5, 2.0, n) / n


def plummer_cloud(n):
    from cstone_amd.clouds import plummer_reference

    x, y, z = plummer_reference(n, "cpu")
    return x.numpy(), y.numpy(), z.numpy(), np.full(n, 1.0 / n)


def uniform_cloud(n, seed):
    rng = np.random.default_rng(seed)
    x, y, z = rng.uniform(0, 1, (3, n))
    return x, y, z, np.full(n, 1.0 / n)


def grav_domain(hip, x, y, z, m, rb=64, mass_bits=64, theta=0.5, kb=64, bucket_focus=64, bc=(0, 0, 0), bucket=None,
                curve=None):
    """a single-rank domain after sync_grav of the cloud: (domain, xd, yd, zd, md) with the synced device arrays"""
    import torch

    import cstone_amd
    from cstone_amd.domain import Domain

    n = x.size
    rdt = np.float64 if rb == 64 else np.float32
    tdt = torch.float64 if rb == 64 else torch.float32
    lo, hi = float(min(a.min() for a in (x, y, z))), float(max(a.max() for a in (x, y, z)))
    lim = [lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo)] * 3  # (an open box is measured by the first sync anyway)
    bucket = 64 * bucket_focus if bucket is None else bucket
    curve = cstone_amd.HILBERT if curve is None else curve
    dom = Domain(hip, curve, kb, rb, bucket, bucket_focus, theta, cstone_amd.make_cbox(lim, bc))
    t = [torch.from_numpy(a.astype(rdt)).cuda() for a in (x, y, z)]
    h = torch.full((n,), 0.01, dtype=tdt, device="cuda")
    mbuf = torch.zeros(n * (rb // mass_bits), dtype=torch.float64 if mass_bits == 64 else torch.float32, device="cuda")
    mbuf[:n] = torch.from_numpy(m.astype(np.float64 if mass_bits == 64 else np.float32)).cuda()
    keys = torch.zeros(n, dtype=torch.int64 if kb == 64 else torch.int32, device="cuda")
    scratch = [torch.empty_like(t[0]) for _ in range(3)]
    keys, xd, yd, zd, hd, md, scratch, _ = dom.sync_grav(keys, *t, h, mbuf[:n], scratch)
    return dom, xd, yd, zd, md


def tree_state(hip, dom, xd, yd, zd, md, kb=64):
    """host copies of the focus tree, the expansion centres and the multipoles (cstone_hip_upsweep_multipoles), and the
    device tensors compute_gravity takes"""
    import torch

    v = dom.view()
    L, M = v.num_focus_leaves, v.num_focus_nodes
    rdt = np.float64 if xd.element_size() == 8 else np.float32
    s = dict(rdt=rdt, L=L, M=M, view=v)
    s["child_offsets"] = dom.fetch(v.child_offsets, M + 1, np.int32)
    s["internal_to_leaf"] = dom.fetch(v.internal_to_leaf, M, np.int32)
    s["leaf_to_internal"] = dom.fetch(v.leaf_to_internal, M, np.int32)
    s["layout"] = dom.fetch(v.layout, L + 1, np.uint32).astype(np.int64)
    s["level_range"] = dom.fetch(v.level_range, MAX_LEVEL[kb] + 2, np.int32)
    s["leaves"] = dom.fetch(v.focus_leaves, L + 1, np.uint64 if kb == 64 else np.uint32)
    assert v.expansion_centers
    s["centers"] = dom.fetch(v.expansion_centers, 4 * M, rdt).reshape(M, 4)
    dev = {k: torch.from_numpy(np.ascontiguousarray(s[k])).cuda() for k in
           ("child_offsets", "internal_to_leaf", "centers")}
    dev["layout"] = torch.from_numpy(s["layout"].astype(np.int32)).cuda()
    dev["lti_leaves"] = torch.from_numpy(np.ascontiguousarray(s["leaf_to_internal"][M - L:])).cuda()
    dev["leaves"] = torch.from_numpy(s["leaves"].view(np.int64 if kb == 64 else np.int32).copy()).cuda()
    mp = hip.upsweep_multipoles(xd, yd, zd, md, dev["lti_leaves"], dev["layout"], s["level_range"],
                                dev["child_offsets"], dev["centers"])
    hip.sync()
    s["multipoles"] = mp.cpu().numpy()
    s["x"], s["y"], s["z"] = [a.cpu().numpy() for a in (xd, yd, zd)]
    s["m"] = md.cpu().numpy()
    s["dev"] = dev
    s["dev"]["multipoles"] = mp
    return s


def groups_of(hip, s, xd, yd, zd):
    import cstone_amd

    n = s["view"].end_index
    return hip.compute_group_splits(0, n, xd, yd, zd, s["dev"]["leaves"], s["dev"]["layout"], s["view"].box, 64,
                                    cstone_amd.GRAVITY_GROUP_TOL)


def gpu_gravity(hip, s, xd, yd, zd, md, groups, order=2, G=1.0, eps2=0.0, counts=True):
    d = s["dev"]
    n = s["view"].end_index
    ax, ay, az, phi, p2p, m2pc = hip.compute_gravity(xd, yd, zd, md, 0, n, groups, s["view"].box, d["child_offsets"],
                                                     d["internal_to_leaf"], d["layout"], d["centers"], d["multipoles"],
                                                     order=order, G=G, eps2=eps2, counts=counts)
    a = np.stack([t.cpu().numpy().astype(np.float64) for t in (ax, ay, az)], 1)
    out = [a, phi.cpu().numpy().astype(np.float64)]
    if counts:
        out += [p2p.cpu().numpy().astype(np.int64), m2pc.cpu().numpy().astype(np.int64)]
    return out


def rel_err(a, ref):
    return np.linalg.norm(a - ref, axis=1) / np.linalg.norm(ref, axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def _compile():
    lib = os.path.join(ROOT, "cornerstone-octree_amd", "lib")
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ["g++", "-std=c++20", "-O1", "-Wall", "-Wno-comment", "-I", os.path.join(ROOT, "include"), "-I",
           os.path.join(ROOT, "cornerstone-octree_amd", "include"), os.path.join(ROOT, "examples", "gravity_example.cpp"),
           "-L", lib, "-lcstone_hip", f"-Wl,-rpath,{lib}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", EXE]
    subprocess.run(cmd, check=True, capture_output=True)


def test_gravity_example_compiles():
    """Domain::computeGravity of the C++ layer, with a plain host compiler against the C ABI"""
    _compile()
    assert os.path.exists(EXE)


def test_gravity_entry_points_are_exported():
    import cstone_amd

    lib = cstone_amd.load_library()
    for name in ("cstone_hip_upsweep_multipoles", "cstone_hip_compute_gravity", "cstone_hip_domain_compute_gravity"):
        assert name in cstone_amd.EXPORTS and hasattr(lib, name)


def test_restated_walk_of_a_single_leaf_is_the_direct_sum():
    """the NumPy restatement itself: a one-leaf tree opens its root and sums every particle (no GPU)"""
    rng = np.random.default_rng(3)
    n = 50
    x, y, z = rng.uniform(0, 1, (3, n))
    m = rng.uniform(0.5, 1.5, n)
    s = dict(rdt=np.float64, x=x, y=y, z=z, m=m, centers=np.array([[0.5, 0.5, 0.5, 4.0]]),
             child_offsets=np.zeros(2, dtype=np.int32), internal_to_leaf=np.zeros(1, dtype=np.int32),
             layout=np.array([0, n]), multipoles=np.zeros((1, 8)))
    a, phi, p2p, m2pc = walk_reference(s, 0, n, 2, eps2=1e-4)
    ra, rphi = direct_sum(x, y, z, m, np.arange(n), eps2=1e-4)
    assert np.allclose(a, ra, rtol=1e-13, atol=0) and np.allclose(phi, rphi, rtol=1e-13)
    assert (p2p == n - 1).all() and (m2pc == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rb,mass_bits", [(64, 64), (64, 32), (32, 32)])
def test_upsweep_multipoles_equal_the_direct_formula(hip, rb, mass_bits):
    """M of every node = the sum of the masses of its particle range, Q = the direct formula about its expansion centre.
    f32: a node around one isotropic blob has a traceless Q about ten times smaller than its terms, and the float
    rounding of the leaf offsets and of the shifts shows at about 1.2e-4 of it (measured on the MI355X; f64: 6e-13), so
    the f32 bound is 3e-4"""
    x, y, z, m = clustered_cloud(40000, 11)
    dom, xd, yd, zd, md = grav_domain(hip, x, y, z, m, rb, mass_bits, bucket_focus=16)
    s = tree_state(hip, dom, xd, yd, zd, md)
    M, child, lr = s["M"], s["child_offsets"], s["level_range"]
    # particle range of every node: leaves from the layout, internal nodes from their first and last child
    lo, hi = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64)
    leaf_nodes = s["leaf_to_internal"][M - s["L"]:]
    lo[leaf_nodes], hi[leaf_nodes] = s["layout"][:-1], s["layout"][1:]
    for level in range(MAX_LEVEL[64], -1, -1):
        for nd in range(lr[level], lr[level + 1]):
            if child[nd]:
                lo[nd], hi[nd] = lo[child[nd]], hi[child[nd] + 7]
    X = np.stack([s["x"], s["y"], s["z"]], 1).astype(np.float64)
    mm = s["m"].astype(np.float64)
    tol = 1e-10 if rb == 64 else 3e-4
    worst = 0.0
    for nd in range(M):
        r = slice(lo[nd], hi[nd])
        got = s["multipoles"][nd].astype(np.float64)
        assert abs(got[0] - mm[r].sum()) <= tol * max(abs(mm[r]).sum(), 1e-300), (nd, got[0], mm[r].sum())
        d = X[r] - s["centers"][nd, :3].astype(np.float64)
        d2 = (d * d).sum(1)
        q = [(mm[r] * (3 * d[:, a] * d[:, b] - (d2 if a == b else 0))).sum() for a, b in
             ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
        scale = max(np.abs(q).max(), 1e-300)
        err = np.abs(got[1:7] - q).max() / scale
        worst = max(worst, err if np.abs(q).max() > 0 else 0.0)
        assert err <= tol or np.abs(q).max() == 0 and np.abs(got[1:7]).max() == 0, (nd, err)
        assert got[7] == 0
    print(f"upsweep rb={rb} mass_bits={mass_bits}: {M} nodes, worst relative |dQ| {worst:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("rb", [64, 32])
def test_walk_equals_the_restatement_exactly(hip, rb):
    """per-target P2P / M2P counts equal the NumPy restatement's exactly (same group boxes, same MAC arithmetic, no
    contraction); accelerations and potentials to rounding (only the order of the sums differs): measured on the MI355X
    6e-15 in f64, 4.3e-6 (a) and 2.7e-6 (phi) in f32, so the f32 bound is 2e-5"""
    x, y, z, m = clustered_cloud(40000, 12)
    dom, xd, yd, zd, md = grav_domain(hip, x, y, z, m, rb, rb, theta=0.5, bucket_focus=16)
    s = tree_state(hip, dom, xd, yd, zd, md)
    groups = groups_of(hip, s, xd, yd, zd)
    eps2 = 1e-6
    a, phi, p2p, m2pc = gpu_gravity(hip, s, xd, yd, zd, md, groups, order=2, G=0.7, eps2=eps2)
    g = groups.cpu().numpy().astype(np.int64)
    assert g[0] == 0 and g[-1] == s["view"].end_index and (np.diff(g) <= 64).all()
    rng = np.random.default_rng(1)
    tol = 1e-10 if rb == 64 else 2e-5
    worst_a = worst_p = 0.0
    for k in rng.choice(g.size - 1, 60, replace=False):
        ra, rphi, rp2p, rm2p = walk_reference(s, g[k], g[k + 1], 2, G=0.7, eps2=eps2)
        sl = slice(g[k], g[k + 1])
        assert np.array_equal(p2p[sl], rp2p), k
        assert np.array_equal(m2pc[sl], rm2p), k
        worst_a = max(worst_a, rel_err(a[sl], ra).max())
        worst_p = max(worst_p, (np.abs(phi[sl] - rphi) / np.abs(rphi)).max())
    print(f"walk rb={rb}: worst relative |da| {worst_a:.2e}, |dphi| {worst_p:.2e}; "
          f"mean P2P {p2p.mean():.0f} M2P {m2pc.mean():.0f} per target")
    assert worst_a <= tol and worst_p <= tol
    assert (m2pc > 0).all() and (p2p > 0).all()


@pytest.mark.gpu
def test_opening_everything_is_the_direct_sum(hip):
    """theta small enough that every non-empty node opens: no M2P, n - 1 P2P per target, the direct sum"""
    x, y, z, m = clustered_cloud(20000, 13)
    dom, xd, yd, zd, md = grav_domain(hip, x, y, z, m, theta=1e-6, bucket_focus=32)
    s = tree_state(hip, dom, xd, yd, zd, md)
    groups = groups_of(hip, s, xd, yd, zd)
    eps2 = 1e-4
    a, phi, p2p, m2pc = gpu_gravity(hip, s, xd, yd, zd, md, groups, eps2=eps2)
    n = x.size
    assert (m2pc == 0).all() and (p2p == n - 1).all()
    tg = np.random.default_rng(2).choice(n, 4096, replace=False)
    ra, rphi = direct_sum(s["x"], s["y"], s["z"], s["m"], tg, eps2=eps2)
    assert rel_err(a[tg], ra).max() <= 1e-10
    assert (np.abs(phi[tg] - rphi) / np.abs(rphi)).max() <= 1e-10


# Figures of this test on the MI355X (n = 40000, theta = 0.5, f64, 4096 targets; relative |da| against the direct sum):
#   plummer  monopole median 9.1e-04  quadrupole median 5.1e-05  p99 2.3e-04
#   uniform  monopole median 4.3e-04  quadrupole median 1.2e-04  p99 8.3e-04
# and relative |dphi|:
#   plummer  monopole median 2.2e-04  quadrupole median 6.5e-06  p99 3.8e-05
#   uniform  monopole median 4.0e-05  quadrupole median 9.3e-06  p99 3.8e-05
# (10^6 Plummer, 512 targets: quadrupole median 1.0e-04, p99 4.7e-04)
@pytest.mark.gpu
@pytest.mark.parametrize("cloud", ["plummer", "uniform"])
def test_accuracy_against_the_direct_sum(hip, cloud):
    n = 40000
    x, y, z, m = plummer_cloud(n) if cloud == "plummer" else uniform_cloud(n, 14)
    dom, xd, yd, zd, md = grav_domain(hip, x, y, z, m, theta=0.5)
    s = tree_state(hip, dom, xd, yd, zd, md)
    groups = groups_of(hip, s, xd, yd, zd)
    tg = np.random.default_rng(4).choice(n, 4096, replace=False)
    ra, rphi = direct_sum(s["x"], s["y"], s["z"], s["m"], tg)
    e, ep = {}, {}
    for order in (0, 2):
        a, phi, _, _ = gpu_gravity(hip, s, xd, yd, zd, md, groups, order=order)
        e[order] = rel_err(a[tg], ra)
        ep[order] = np.abs(phi[tg] - rphi) / np.abs(rphi)
    med0, med2, p99 = np.median(e[0]), np.median(e[2]), np.percentile(e[2], 99)
    pmed0, pmed2, pp99 = np.median(ep[0]), np.median(ep[2]), np.percentile(ep[2], 99)
    print(f"{cloud}: monopole median {med0:.1e}  quadrupole median {med2:.1e}  p99 {p99:.1e}; potential: monopole "
          f"median {pmed0:.1e}  quadrupole median {pmed2:.1e}  p99 {pp99:.1e}")
    assert med2 < med0
    assert med2 <= 1e-3 and p99 <= 1e-2
    assert pmed2 < pmed0
    assert pmed2 <= 5e-5 and pp99 <= 2e-4


@pytest.mark.gpu
def test_domain_gravity_equals_compute_gravity_and_refuses(hip):
    """Domain.gravity after sync_grav = compute_gravity on the view's arrays bit for bit; CSTONE_E_ARG before sync_grav,
    after a plain sync and for a periodic box"""
    import torch

    import cstone_amd
    from cstone_amd import CstoneError

    x, y, z, m = clustered_cloud(30000, 15)
    for rb in (64, 32):
        dom, xd, yd, zd, md = grav_domain(hip, x, y, z, m, rb, 32)
        s = tree_state(hip, dom, xd, yd, zd, md)
        groups = groups_of(hip, s, xd, yd, zd)
        for order in (0, 2):
            a, phi = gpu_gravity(hip, s, xd, yd, zd, md, groups, order=order, G=2.0, eps2=1e-4, counts=False)
            ax, ay, az, ph = dom.gravity(xd, yd, zd, md, G=2.0, eps=1e-2, order=order)
            got = np.stack([t.cpu().numpy().astype(np.float64) for t in (ax, ay, az)], 1)
            assert np.array_equal(got, a) and np.array_equal(ph.cpu().numpy().astype(np.float64), phi), (rb, order)
        assert dom.gravity(xd, yd, zd, md, potential=False)[3] is None
        # a plain sync drops the expansion centres
        n = xd.numel()
        t = [a.clone() for a in (xd, yd, zd)]
        keys = torch.zeros(n, dtype=torch.int64, device="cuda")
        dom.sync(keys, *t, torch.full_like(t[0], 0.01), [torch.empty_like(t[0]) for _ in range(3)])
        with pytest.raises(CstoneError, match=r"\(-1\)"):
            dom.gravity(*t, md)
    from cstone_amd.domain import Domain

    fresh = Domain(hip, cstone_amd.HILBERT, 64, 64, 1024, 64, 0.5, cstone_amd.make_cbox([0, 1] * 3))
    xd = torch.from_numpy(x).cuda()
    with pytest.raises(CstoneError, match=r"\(-1\)"):
        fresh.gravity(xd, xd, xd, xd)
    pdom, xd, yd, zd, md = grav_domain(hip, x, y, z, m, bc=(1, 1, 1))
    assert pdom.view().expansion_centers
    with pytest.raises(CstoneError, match=r"\(-1\)"):
        pdom.gravity(xd, yd, zd, md)


@pytest.mark.gpu
def test_gravity_example_prints_the_python_accelerations(hip):
    """examples/gravity_example.cpp (Domain::computeGravity of the C++ layer) against Domain.gravity on the same cloud"""
    if not os.path.exists(EXE):
        _compile()
    n = 20000
    out = subprocess.run([EXE, str(n)], check=True, capture_output=True, text=True, timeout=120).stdout
    rows = [line.split() for line in out.splitlines() if line.startswith("row ")]
    assert len(rows) == 4, out
    i = np.arange(n, dtype=np.float64)
    x = np.fmod(i * 0.7548776662466927 + 0.1, 1.0)
    y = np.fmod(i * 0.5698402909980532 + 0.2, 1.0)
    z = np.fmod(i * 0.3819660112501051 + 0.3, 1.0)
    m = np.full(n, 1.0 / n)
    dom, xd, yd, zd, md = grav_domain(hip, x, y, z, m, theta=0.5, bucket_focus=64, bucket=1024)
    ax, ay, az, phi = dom.gravity(xd, yd, zd, md, G=1.0, eps=0.01)
    got = np.stack([t.cpu().numpy() for t in (ax, ay, az, phi)], 1)
    for r in rows:
        k = int(r[1])
        assert np.allclose([float(v) for v in r[2:6]], got[k], rtol=1e-12, atol=0), (r, got[k])


@pytest.mark.gpu
def test_a_million_plummer_particles(hip):
    """10^6 Plummer particles, f64: no error-word bit, 512 sampled targets within the accuracy bounds"""
    n = 1000000
    x, y, z, m = plummer_cloud(n)
    dom, xd, yd, zd, md = grav_domain(hip, x, y, z, m, theta=0.5)
    ax, ay, az, _ = dom.gravity(xd, yd, zd, md, potential=False)
    hip.sync()  # (the sticky error word: raises if any bit is set)
    a = np.stack([t.cpu().numpy() for t in (ax, ay, az)], 1)
    tg = np.random.default_rng(5).choice(n, 512, replace=False)
    ra, _ = direct_sum(xd.cpu().numpy(), yd.cpu().numpy(), zd.cpu().numpy(), md.cpu().numpy(), tg)
    e = rel_err(a[tg], ra)
    print(f"1e6 plummer: median {np.median(e):.1e} p99 {np.percentile(e, 99):.1e}")
    assert np.median(e) <= 1e-3 and np.percentile(e, 99) <= 1e-2
