"""Gravity (csrc/gravity.hip) against independent references, on hand-built trees and through the Domain.

The hand-built trees reach what a Domain never builds: groups longer than 64 targets, sub-ranges [first, last) that
cut through groups, targets that belong to no leaf, leaves of more than 64 particles, nodes skipped for macSq == 0, the
deepest tree the walk's stack is sized for, and the (f32 coordinates, f64 masses) instantiations.  The M2P expansion is
judged by its convergence order against the direct sum and by force = -grad(potential), neither of which shares a
formula with the kernel or with the NumPy restatement of test_gravity.py."""
import ctypes as C

import numpy as np
import pytest

from test_gravity import (clustered_cloud, direct_sum, grav_domain, groups_of, gpu_gravity, rel_err,
                          tree_state, walk_reference)

HUGE_MAC = 1e30  # a MAC radius^2 that opens every node


# ---------------------------------------------------------------------------------------------------------------------
# hand-built trees (host side)
# ---------------------------------------------------------------------------------------------------------------------
def build_tree(desc):
    """the linked-octree arrays of a nested description: a leaf is an int (its number of source particles), an internal
    node a list of 8 descriptions.  Nodes are numbered level by level (root 0, the 8 children of a node contiguous, in
    order), leaves and their particles in depth-first order, as in tree_state().  Returns a dict with child_offsets
    (M + 1), internal_to_leaf (M, -1 for internal nodes), leaf_to_internal (the L leaf entries), layout (L + 1),
    level_range (levels + 1), and per node its particle range (lo, hi), level and octant path from the root"""
    nodes, paths, levels = [desc], [()], [0]
    child = []
    k = 0
    while k < len(nodes):  # breadth first: the numbering is level-ordered and children are contiguous
        d = nodes[k]
        if isinstance(d, list):
            assert len(d) == 8
            child.append(len(nodes))
            nodes += d
            paths += [paths[k] + (o,) for o in range(8)]
            levels += [levels[k] + 1] * 8
        else:
            child.append(0)
        k += 1
    M = len(nodes)
    child_offsets = np.zeros(M + 1, dtype=np.int32)
    child_offsets[:M] = child
    lo, hi = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64)
    itl = np.full(M, -1, dtype=np.int32)
    lti, layout = [], [0]

    def dfs(n):  # leaves and particles in depth-first (space-filling-curve) order
        lo[n] = layout[-1]
        if child[n] == 0:
            itl[n] = len(lti)
            lti.append(n)
            layout.append(layout[-1] + nodes[n])
        else:
            for c in range(child[n], child[n] + 8):
                dfs(c)
        hi[n] = layout[-1]

    dfs(0)
    levels = np.array(levels)
    depth = levels.max()
    level_range = np.array([np.searchsorted(levels, lv) for lv in range(depth + 2)], dtype=np.int32)
    return dict(child_offsets=child_offsets, internal_to_leaf=itl, leaf_to_internal=np.array(lti, dtype=np.int32),
                layout=np.array(layout, dtype=np.int64), level_range=level_range, lo=lo, hi=hi, level=levels,
                paths=paths, M=M, L=len(lti), n_src=int(layout[-1]))


def cube_of(path, origin=(0.0, 0.0, 0.0), size=1.0):
    """lower corner and edge of the cube of an octant path (octant o: x from bit 2, y from bit 1, z from bit 0)"""
    c = np.array(origin, dtype=np.float64)
    for o in path:
        size *= 0.5
        c += size * np.array([(o >> 2) & 1, (o >> 1) & 1, o & 1])
    return c, size


def place_sources(tr, rng, mass=(0.5, 1.5)):
    """x, y, z, m of the sources, uniform in their leaf's cube, in layout order"""
    pos = np.zeros((tr["n_src"], 3))
    for lf, n in enumerate(tr["leaf_to_internal"]):
        c, s = cube_of(tr["paths"][n])
        a, b = tr["layout"][lf], tr["layout"][lf + 1]
        pos[a:b] = c + s * rng.uniform(0.05, 0.95, (b - a, 3))
    return pos[:, 0], pos[:, 1], pos[:, 2], rng.uniform(*mass, tr["n_src"])


def centers_of(tr, x, y, z, m, mac):
    """(M, 4) float64: the centre of mass of every node's particles and [3] = mac(node) (0 for a massless node, as
    set_mac leaves it; such a node gets its cube's centre)"""
    ctr = np.zeros((tr["M"], 4))
    for n in range(tr["M"]):
        r = slice(tr["lo"][n], tr["hi"][n])
        w = m[r].sum()
        if w > 0:
            ctr[n, :3] = [(m[r] * a[r]).sum() / w for a in (x, y, z)]
            ctr[n, 3] = mac(n)
        else:
            c, s = cube_of(tr["paths"][n])
            ctr[n, :3] = c + 0.5 * s
    return ctr


def geometric_mac(tr, theta):
    """(edge * sqrt(3) / theta)^2 of every node's cube: opens nodes near the targets, accepts far ones"""
    return lambda n: (cube_of(tr["paths"][n])[1] * np.sqrt(3.0) / theta) ** 2


def direct_multipoles(tr, x, y, z, m, ctr):
    """(M, 8) float64: M and the traceless quadrupole of every node's particles about its centre, the direct formula"""
    X = np.stack([x, y, z], 1).astype(np.float64)
    mm = np.asarray(m, dtype=np.float64)
    out = np.zeros((tr["M"], 8))
    for n in range(tr["M"]):
        r = slice(tr["lo"][n], tr["hi"][n])
        d = X[r] - np.asarray(ctr[n, :3], dtype=np.float64)
        d2 = (d * d).sum(1)
        out[n, 0] = mm[r].sum()
        out[n, 1:7] = [(mm[r] * (3 * d[:, a] * d[:, b] - (d2 if a == b else 0))).sum() for a, b in
                       ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return out


def sources_only(m, n_src):
    """the masses with those of the targets that belong to no leaf set to 0: direct_sum over the sources alone"""
    w = np.array(m, dtype=np.float64)
    w[n_src:] = 0.0
    return w


def force_scale(x, y, z, m, n_src, targets, eps2=0.0):
    """G sum_j m_j / (r_ij^2 + eps2) over the sources: the size of the terms of the force on each target, the scale of
    the rounding of a float32 sum whatever cancels in it"""
    X = np.stack([x, y, z], 1).astype(np.float64)
    w = np.asarray(m, dtype=np.float64)[:n_src]
    out = np.zeros(len(targets))
    for k, i in enumerate(targets):
        r2 = ((X[:n_src] - X[i]) ** 2).sum(1) + eps2
        keep = np.arange(n_src) != i
        out[k] = (w[keep] / r2[keep]).sum()
    return out


def restatement_state(tr, x, y, z, m, ctr, mp, rdt):
    """the dict walk_reference() reads, for a hand-built tree"""
    return dict(rdt=rdt, x=np.asarray(x, dtype=rdt), y=np.asarray(y, dtype=rdt), z=np.asarray(z, dtype=rdt),
                m=np.asarray(m), centers=np.asarray(ctr, dtype=rdt), child_offsets=tr["child_offsets"],
                internal_to_leaf=tr["internal_to_leaf"], layout=tr["layout"], multipoles=np.asarray(mp))


# three levels below the root, a mix of internal nodes and leaves of 0 .. 29 particles (some empty)
def three_level_desc(seed=21):
    rng = np.random.default_rng(seed)

    def leaves():
        return [int(v) for v in rng.integers(0, 20, 8)]

    lvl2 = leaves()
    lvl2[5] = leaves()  # a third level
    desc = [int(v) for v in rng.integers(0, 30, 8)]
    desc[0], desc[3], desc[6] = leaves(), lvl2, leaves()
    return desc


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the builder and the restatement
# ---------------------------------------------------------------------------------------------------------------------
def test_builder_numbers_nodes_level_by_level():
    tr = build_tree(three_level_desc())
    M, L = tr["M"], tr["L"]
    child, lv, lr = tr["child_offsets"], tr["level"], tr["level_range"]
    assert M == L + (L - 1) // 7 and M == 1 + 8 * 5 and L == M - 5
    assert list(lr) == [0, 1, 9, 33, 41] and (np.diff(lv) >= 0).all()
    internal = np.nonzero(child[:M])[0]
    assert list(lv[internal]) == [0, 1, 1, 1, 2]
    for n in internal:  # 8 contiguous children one level down; an internal node spans its children's particles
        assert (lv[child[n]:child[n] + 8] == lv[n] + 1).all()
        assert tr["lo"][n] == tr["lo"][child[n]] and tr["hi"][n] == tr["hi"][child[n] + 7]
    assert sorted(np.concatenate([[0], (child[internal, None] + np.arange(8)).ravel()])) == list(range(M))
    lti, itl, layout = tr["leaf_to_internal"], tr["internal_to_leaf"], tr["layout"]
    assert (itl[lti] == np.arange(L)).all() and (itl[internal] == -1).all()
    assert (np.diff(layout) >= 0).all() and layout[0] == 0 and layout[-1] == tr["n_src"]
    assert (tr["lo"][lti] == layout[:-1]).all() and (tr["hi"][lti] == layout[1:]).all()
    # the leaves' cubes tile the root's cube, in depth-first order of the octant paths
    assert sum(cube_of(tr["paths"][n])[1] ** 3 for n in lti) == 1.0
    assert [tr["paths"][n] for n in lti] == sorted(tr["paths"][n] for n in lti)


def test_builder_of_the_deepest_chain():
    tr = build_tree(chain_desc(21, 2))
    assert tr["M"] == 169 and tr["L"] == 148 and len(tr["level_range"]) == 23 and tr["level"].max() == 21
    assert tr["n_src"] == 2 * 148


def test_restated_long_groups_are_the_direct_sum():
    """groups of up to 200 targets (4 runs of 64), sources and targets that belong to no leaf: with every node opened
    the restatement is the direct sum over the sources, n_src - 1 P2P per source and n_src per other target"""
    tr = build_tree(three_level_desc())
    rng = np.random.default_rng(5)
    x, y, z, m = place_sources(tr, rng)
    ns, ne = tr["n_src"], 60
    x, y, z = [np.concatenate([a, rng.uniform(0, 1, ne)]) for a in (x, y, z)]
    m = np.concatenate([m, rng.uniform(0.5, 1.5, ne)])  # (targets' masses: never read)
    ctr = centers_of(tr, x, y, z, m, lambda n: HUGE_MAC)
    t = restatement_state(tr, x, y, z, m, ctr, np.zeros((tr["M"], 8)), np.float64)
    bounds = [0, 1, 64, 129, 130, 330, ns + ne]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        a, phi, p2p, m2pc = walk_reference(t, lo, hi, 2, G=0.5, eps2=1e-5)
        tg = np.arange(lo, hi)
        ra, rphi = direct_sum(x, y, z, sources_only(m, ns), tg, G=0.5, eps2=1e-5)
        assert a.shape == (hi - lo, 3) and np.allclose(a, ra, rtol=1e-12, atol=0)
        assert np.allclose(phi, rphi, rtol=1e-12, atol=0)
        assert (p2p == np.where(tg < ns, ns - 1, ns)).all() and (m2pc == 0).all()


def test_restated_long_group_takes_one_box_per_run():
    """the runs of a long group are walked with their own boxes: a group whose first 64 targets sit in one corner and
    the rest in the opposite corner accepts nodes in both runs, which one box around all 128 targets could not (it would
    hold every node's centre, and open every node)"""
    tr = build_tree([3] * 8)
    rng = np.random.default_rng(6)
    x, y, z, m = place_sources(tr, rng)
    ns = tr["n_src"]
    pts = np.concatenate([np.stack([x, y, z], 1), rng.uniform(0.0, 0.05, (64, 3)), rng.uniform(0.95, 1.0, (64, 3))])
    x, y, z = pts.T
    m = np.concatenate([m, np.zeros(128)])
    ctr = centers_of(tr, x, y, z, m, lambda n: 0.8 ** 2 if n else HUGE_MAC)
    assert ((ctr[:, :3] > 0.05) & (ctr[:, :3] < 0.95)).all()
    t = restatement_state(tr, x, y, z, m, ctr, direct_multipoles(tr, x, y, z, m, ctr), np.float64)
    whole = walk_reference(t, ns, ns + 128, 2)
    runs = [walk_reference(t, lo, lo + 64, 2) for lo in (ns, ns + 64)]
    for w, r in zip(whole, zip(*runs)):
        assert np.array_equal(w, np.concatenate(r))
    assert (whole[3] > 0).all() and (whole[2] > 0).all()


def test_direct_multipoles_shift_like_the_parallel_axis_theorem():
    """the direct formula of the hand-built trees: a parent's Q equals its children's Q shifted to its centre"""
    tr = build_tree(three_level_desc())
    x, y, z, m = place_sources(tr, np.random.default_rng(7))
    ctr = centers_of(tr, x, y, z, m, lambda n: 1.0)
    mp = direct_multipoles(tr, x, y, z, m, ctr)
    for n in np.nonzero(tr["child_offsets"][:tr["M"]])[0]:
        q = np.zeros(7)
        for c in range(tr["child_offsets"][n], tr["child_offsets"][n] + 8):
            s = ctr[c, :3] - ctr[n, :3]
            s2 = s @ s
            mc = mp[c, 0]
            q += mp[c, :7] + mc * np.array([0, 3 * s[0] * s[0] - s2, 3 * s[0] * s[1], 3 * s[0] * s[2],
                                            3 * s[1] * s[1] - s2, 3 * s[1] * s[2], 3 * s[2] * s[2] - s2])
        assert np.allclose(q, mp[n, :7], rtol=1e-12, atol=1e-12 * np.abs(mp[n, :7]).max())


def chain_desc(depth, per_leaf):
    """node 0 of every level internal down to `depth`, the other 7 nodes of each level leaves"""
    return per_leaf if depth == 0 else [chain_desc(depth - 1, per_leaf)] + [per_leaf] * 7


# ---------------------------------------------------------------------------------------------------------------------
# GPU: hand-built trees through the context API
# ---------------------------------------------------------------------------------------------------------------------
def upload(hip, tr, x, y, z, m, ctr, rb=64, mb=64):
    """device tensors of a hand-built tree and its particles (coordinates and centres in rb bits, masses in mb)"""
    import torch

    rdt, mdt = (np.float64 if rb == 64 else np.float32), (np.float64 if mb == 64 else np.float32)

    def dev(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()

    return dict(rb=rb, mb=mb, rdt=rdt, x=dev(x, rdt), y=dev(y, rdt), z=dev(z, rdt), m=dev(m, mdt),
                centers=dev(ctr, rdt), child_offsets=dev(tr["child_offsets"], np.int32),
                internal_to_leaf=dev(tr["internal_to_leaf"], np.int32), lti=dev(tr["leaf_to_internal"], np.int32),
                layout=dev(tr["layout"], np.int32), level_range=tr["level_range"])


def upsweep(hip, d):
    mp = hip.upsweep_multipoles(d["x"], d["y"], d["z"], d["m"], d["lti"], d["layout"], d["level_range"],
                                d["child_offsets"], d["centers"])
    hip.sync()
    return mp


def raw_gravity(hip, d, mp, first, last, groups, order=2, G=1.0, eps2=0.0):
    """cstone_hip_compute_gravity called directly, its outputs pre-filled with NaN and the counts with 0xffffffff:
    (return code, a (last - first, 3), phi, p2p, m2p) as float64 / int64, untouched slots still NaN / -1"""
    import torch

    import cstone_amd
    from cstone_amd import _ptr

    nt = last - first
    dt = d["x"].dtype
    ax, ay, az, phi = [torch.full((nt,), float("nan"), dtype=dt, device="cuda") for _ in range(4)]
    p2p, m2pc = [torch.full((nt,), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
    g = torch.from_numpy(np.asarray(groups, dtype=np.int32)).cuda()
    box = cstone_amd.make_cbox([-4.0, 4.0] * 3)
    rc = hip.lib.cstone_hip_compute_gravity(
        hip.h, C.c_int(d["rb"]), C.c_int(d["mb"]), _ptr(d["x"]), _ptr(d["y"]), _ptr(d["z"]), _ptr(d["m"]),
        C.c_uint32(first), C.c_uint32(last), _ptr(g), C.c_uint32(g.numel() - 1), C.byref(box), _ptr(d["child_offsets"]),
        _ptr(d["internal_to_leaf"]), _ptr(d["layout"]), _ptr(d["centers"]), _ptr(mp), C.c_int(order), C.c_double(G),
        C.c_double(eps2), _ptr(ax), _ptr(ay), _ptr(az), _ptr(phi), _ptr(p2p), _ptr(m2pc))
    hip.sync()
    a = np.stack([t.cpu().numpy().astype(np.float64) for t in (ax, ay, az)], 1)
    return (rc, a, phi.cpu().numpy().astype(np.float64), p2p.cpu().numpy().astype(np.int64),
            m2pc.cpu().numpy().astype(np.int64))


def one_node_cluster(n=400, seed=31):
    """an elongated, bent ellipsoid of random masses (large Q and octupole), its centre of mass at the origin"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u *= (rng.uniform(0, 1, n) ** (1 / 3) / np.linalg.norm(u, axis=1))[:, None]
    p = u * [1.0, 0.4, 0.2]
    p[:, 1] += 0.6 * p[:, 0] ** 2  # bent: the octupole, the first term the quadrupole leaves out, is not small
    m = rng.uniform(0.2, 2.0, n)
    p -= (m[:, None] * p).sum(0) / m.sum()
    return p, m


def directions(k):
    """k unit vectors spread over the sphere (Fibonacci lattice)"""
    i = np.arange(k) + 0.5
    ct = 1 - 2 * i / k
    st = np.sqrt(1 - ct * ct)
    ph = np.pi * (1 + 5 ** 0.5) * i
    return np.stack([st * np.cos(ph), st * np.sin(ph), ct], 1)


def root_m2p_setup(hip, targets, mac=1e-20, rb=64, mb=64):
    """a one-node tree (the root a leaf of the cluster) with a tiny MAC radius: every target takes the root as one M2P.
    Targets come after the sources and are one group each"""
    p, m = one_node_cluster()
    tr = build_tree(len(m))
    pts = np.concatenate([p, targets])
    x, y, z = pts.T
    mm = np.concatenate([m, np.zeros(len(targets))])
    ctr = centers_of(tr, x, y, z, mm, lambda n: mac)
    return tr, x, y, z, mm, ctr


# Slopes of the median relative error against r (r = 4 .. 64 cluster lengths, 16 directions, f64, eps2 = 0).
# Monopole: the dipole about the centre of mass vanishes, so the first neglected term is the quadrupole, r^-2 relative
# for force and potential alike; quadrupole: the octupole, r^-3.  Measured on the MI355X:
#   monopole    force -2.01  potential -2.02   (median error at r = 4: 1.8e-02 / 3.5e-03)
#   quadrupole  force -2.99  potential -3.02   (median error at r = 4: 2.1e-03 / 2.8e-04)
# A wrong factor in the quadrupole terms leaves an r^-2 error behind: the slope of the quadrupole becomes -2.
@pytest.mark.gpu
def test_m2p_converges_at_the_order_of_the_expansion(hip):
    rs = 2.0 ** np.arange(2, 7)
    dirs = directions(16)
    tg = np.concatenate([r * dirs for r in rs])
    tr, x, y, z, m, ctr = root_m2p_setup(hip, tg)
    ns, nt = tr["n_src"], len(tg)
    d = upload(hip, tr, x, y, z, m, ctr)
    mp = upsweep(hip, d)
    ra, rphi = direct_sum(x, y, z, m, np.arange(ns, ns + nt))
    groups = np.arange(ns, ns + nt + 1)
    for order, want in ((0, -2.0), (2, -3.0)):
        rc, a, phi, p2p, m2pc = raw_gravity(hip, d, mp, ns, ns + nt, groups, order=order)
        assert rc == 0 and (p2p == 0).all() and (m2pc == 1).all()
        ea = rel_err(a, ra).reshape(len(rs), -1)
        ep = (np.abs(phi - rphi) / np.abs(rphi)).reshape(len(rs), -1)
        sa = np.polyfit(np.log(rs), np.log(np.median(ea, 1)), 1)[0]
        sp = np.polyfit(np.log(rs), np.log(np.median(ep, 1)), 1)[0]
        print(f"order {order}: slope force {sa:.2f} potential {sp:.2f}; median errors at r = 4: "
              f"{np.median(ea[0]):.1e} / {np.median(ep[0]):.1e}, r = 64: {np.median(ea[-1]):.1e} / {np.median(ep[-1]):.1e}")
        assert abs(sa - want) <= 0.2 and abs(sp - want) <= 0.2, (order, sa, sp)


def grad_check(hip, tr, x, y, z, m, ctr, targets, order, eps2, rel_h):
    """-(central differences of phi) against a, every target shifted by +-h (h = rel_h * |target|) along x, y and z.
    Returns the worst relative difference; the counts of the seven evaluations must be identical"""
    ns, nt = tr["n_src"], len(targets)
    h = rel_h * np.linalg.norm(targets, axis=1)
    groups = np.arange(ns, ns + nt + 1)

    def run(shift):
        pts = targets + shift
        xx, yy, zz = [np.concatenate([s, t]) for s, t in zip((x[:ns], y[:ns], z[:ns]), pts.T)]
        d = upload(hip, tr, xx, yy, zz, m, ctr)
        rc, a, phi, p2p, m2pc = raw_gravity(hip, d, upsweep(hip, d), ns, ns + nt, groups, order=order, eps2=eps2)
        assert rc == 0 and not np.isnan(a).any()
        return a, phi, (p2p, m2pc), pts

    a0, _, counts0, _ = run(np.zeros((nt, 3)))
    g = np.zeros((nt, 3))
    for k in range(3):
        e = np.zeros((nt, 3))
        e[:, k] = h
        _, pp, cp, xp = run(e)
        _, pm, cm, xm = run(-e)
        for c in (cp, cm):
            assert all(np.array_equal(u, v) for u, v in zip(c, counts0))
        g[:, k] = -(pp - pm) / (xp[:, k] - xm[:, k])
    return rel_err(g, a0).max()


# Worst relative |(-grad phi) - a| (h = 1e-5 r: the truncation of the central difference is ~(h / r)^2 = 1e-10, the
# rounding of phi ~1e-16 / 1e-5 = 1e-11), measured on the MI355X: M2P 0.9e-10 .. 1.0e-10, P2P 1.5e-10 .. 1.6e-10.
# A force factor off by 2.5 / 2 or a potential factor off by 2 shows at 1e-3 and more.
@pytest.mark.gpu
@pytest.mark.parametrize("eps2", [0.0, 0.25])
@pytest.mark.parametrize("order", [0, 2])
def test_m2p_force_is_minus_the_gradient_of_its_potential(hip, order, eps2):
    tg = np.concatenate([r * directions(16) for r in (3.0, 12.0)])
    tr, x, y, z, m, ctr = root_m2p_setup(hip, tg)
    worst = grad_check(hip, tr, x, y, z, m, ctr, tg, order, eps2, 1e-5)
    print(f"M2P order {order} eps2 {eps2}: worst relative |grad - a| {worst:.1e}")
    assert worst <= 1e-8


@pytest.mark.gpu
@pytest.mark.parametrize("eps2", [0.0, 0.01])
def test_p2p_force_is_minus_the_gradient_of_its_potential(hip, eps2):
    """every node opened: the P2P sums, targets 1.5 .. 3 from the cloud's centre (outside it)"""
    tr = build_tree(three_level_desc())
    rng = np.random.default_rng(8)
    x, y, z, m = place_sources(tr, rng)
    tg = 0.5 + np.concatenate([r * directions(16) for r in (1.5, 3.0)])
    m = np.concatenate([m, np.zeros(len(tg))])
    # the cloud moved to the origin: h is relative to the distance from its centre
    x, y, z = x - 0.5, y - 0.5, z - 0.5
    ctr = centers_of(tr, x, y, z, m[:tr["n_src"]], lambda n: HUGE_MAC)
    worst = grad_check(hip, tr, x, y, z, m, ctr, tg - 0.5, 2, eps2, 1e-5)
    print(f"P2P eps2 {eps2}: worst relative |grad - a| {worst:.1e}")
    assert worst <= 1e-8


GROUP_LENGTHS = [63, 1, 64, 0, 65, 130, 200]


@pytest.mark.gpu
@pytest.mark.parametrize("rb,mb", [(64, 64), (64, 32), (32, 32), (32, 64)])
@pytest.mark.parametrize("cut", ["through", "around"])
def test_long_and_ragged_groups_and_sub_ranges(hip, rb, mb, cut):
    """groups of 63, 1, 64, 0, 65, 130 and 200 targets on a three-level tree of opened and accepted nodes, sources
    followed by targets in no leaf.  'through': first and last cut through the first and last groups; 'around': they
    lie outside the groups, whose outside targets keep their NaN (the ABI leaves them untouched).  Counts equal the
    restatement's exactly, a and phi to its tolerance"""
    tr = build_tree(three_level_desc())
    rng = np.random.default_rng(9)
    x, y, z, m = place_sources(tr, rng)
    ns, N = tr["n_src"], 555
    assert ns < 500
    x, y, z = [np.concatenate([a, rng.uniform(0, 1, N - ns)]) for a in (x, y, z)]
    rdt, mdt = (np.float64 if rb == 64 else np.float32), (np.float64 if mb == 64 else np.float32)
    m = np.concatenate([m, np.zeros(N - ns)]).astype(mdt).astype(np.float64)  # (the restatement reads these masses)
    xr, yr, zr = [a.astype(rdt) for a in (x, y, z)]
    ctr = centers_of(tr, xr.astype(np.float64), yr.astype(np.float64), zr.astype(np.float64), m,
                     geometric_mac(tr, 0.6))
    d = upload(hip, tr, xr, yr, zr, m, ctr, rb, mb)
    mp = upsweep(hip, d)
    t = restatement_state(tr, xr, yr, zr, m, ctr, mp.cpu().numpy(), rdt)
    g0 = 0 if cut == "through" else 12
    groups = g0 + np.concatenate([[0], np.cumsum(GROUP_LENGTHS)])
    first, last = (17, int(groups[-1]) - 40) if cut == "through" else (4, N)
    eps2, G = 1e-4, 0.8
    rc, a, phi, p2p, m2pc = raw_gravity(hip, d, mp, first, last, groups, 2, G, eps2)
    assert rc == 0
    inside = np.zeros(last - first, dtype=bool)
    tol = 1e-10 if rb == 64 else 5e-6  # f32: 9.7e-7 measured on the MI355X
    worst = 0.0
    for lo, hi in zip(groups[:-1], groups[1:]):
        lo, hi = max(first, lo), min(last, hi)
        if hi <= lo:
            continue
        ra, rphi, rp2p, rm2p = walk_reference(t, lo, hi, 2, G, eps2)
        sl = slice(lo - first, hi - first)
        inside[sl] = True
        assert np.array_equal(p2p[sl], rp2p) and np.array_equal(m2pc[sl], rm2p), (lo, hi)
        scale = G * force_scale(xr, yr, zr, m, ns, np.arange(lo, hi), eps2)
        worst = max(worst, (np.linalg.norm(a[sl] - ra, axis=1) / scale).max(),
                    (np.abs(phi[sl] - rphi) / np.abs(rphi)).max())
    print(f"rb={rb} mb={mb} {cut}: worst relative difference to the restatement {worst:.1e}; "
          f"M2P {m2pc[inside].min()}..{m2pc[inside].max()}, P2P {p2p[inside].min()}..{p2p[inside].max()}")
    assert worst <= tol
    assert (m2pc[inside] > 0).any() and (p2p[inside] > 0).any() and (m2pc[inside] == 0).any()
    assert inside.sum() == (last - first if cut == "through" else groups[-1] - groups[0])
    assert np.isnan(a[~inside]).all() and np.isnan(phi[~inside]).all()
    assert (p2p[~inside] == -1).all() and (m2pc[~inside] == -1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("rb", [64, 32])
def test_leaves_of_more_than_64_particles(hip, rb):
    """every node opened; leaf 1 holds 200 particles starting at 50, so the target itself falls in the 1st .. 4th
    64-particle pass of its own leaf; a leaf of 65 takes a pass of 1.  Direct sum; P2P = n_src - 1 for a source"""
    tr = build_tree([50, 200, 3, 0, 70, 10, 1, 65])
    rng = np.random.default_rng(10)
    x, y, z, m = place_sources(tr, rng)
    ns, ne = tr["n_src"], 30
    x, y, z = [np.concatenate([a, rng.uniform(0, 1, ne)]) for a in (x, y, z)]
    m = np.concatenate([m, np.zeros(ne)])
    rdt = np.float64 if rb == 64 else np.float32
    xr, yr, zr = [a.astype(rdt).astype(np.float64) for a in (x, y, z)]
    ctr = centers_of(tr, xr, yr, zr, m, lambda n: HUGE_MAC)
    d = upload(hip, tr, xr, yr, zr, m, ctr, rb, rb)
    N = ns + ne
    groups = list(range(0, N, 64)) + [N]
    eps2 = 1e-6
    rc, a, phi, p2p, m2pc = raw_gravity(hip, d, upsweep(hip, d), 0, N, groups, 2, 1.0, eps2)
    assert rc == 0
    assert (p2p == np.where(np.arange(N) < ns, ns - 1, ns)).all() and (m2pc == 0).all()
    ra, rphi = direct_sum(xr, yr, zr, m, np.arange(N), eps2=eps2)
    scale = force_scale(xr, yr, zr, m, ns, np.arange(N), eps2)
    ea, ep = (np.linalg.norm(a - ra, axis=1) / scale).max(), (np.abs(phi - rphi) / np.abs(rphi)).max()
    print(f"rb={rb}: worst relative |da| {ea:.1e} |dphi| {ep:.1e}")
    tol = 1e-12 if rb == 64 else 5e-6  # measured on the MI355X: 1.4e-15 / 2.5e-15, f32 5.6e-7 / 9.3e-7
    assert ea <= tol and ep <= tol


@pytest.mark.gpu
def test_a_node_with_mass_and_zero_mac_is_skipped(hip):
    """leaf 2 has particles and mass but macSq = 0: the walk skips it (no contribution, not counted), its particles still
    receive the force of the others.  Everything else opened: the direct sum without leaf 2's masses"""
    tr = build_tree([20, 30, 25, 10, 40, 5, 15, 30])
    rng = np.random.default_rng(12)
    x, y, z, m = place_sources(tr, rng)
    ns = tr["n_src"]
    skipped = tr["leaf_to_internal"][2]
    ctr = centers_of(tr, x, y, z, m, lambda n: 0.0 if n == skipped else HUGE_MAC)
    assert ctr[skipped, 3] == 0 and m[tr["lo"][skipped]:tr["hi"][skipped]].sum() > 0
    d = upload(hip, tr, x, y, z, m, ctr)
    mp = upsweep(hip, d)
    groups = list(range(0, ns, 64)) + [ns]
    rc, a, phi, p2p, m2pc = raw_gravity(hip, d, mp, 0, ns, groups, 2, 1.0, 1e-4)
    assert rc == 0
    in_skipped = (np.arange(ns) >= tr["lo"][skipped]) & (np.arange(ns) < tr["hi"][skipped])
    n_skip = in_skipped.sum()
    assert (p2p == np.where(in_skipped, ns - n_skip, ns - n_skip - 1)).all() and (m2pc == 0).all()
    w = m.copy()
    w[in_skipped] = 0
    ra, rphi = direct_sum(x, y, z, w, np.arange(ns), eps2=1e-4)
    assert rel_err(a, ra).max() <= 1e-12 and (np.abs(phi - rphi) / np.abs(rphi)).max() <= 1e-12
    t = restatement_state(tr, x, y, z, m, ctr, mp.cpu().numpy(), np.float64)
    for lo, hi in zip(groups[:-1], groups[1:]):
        _, _, rp2p, rm2p = walk_reference(t, lo, hi, 2, eps2=1e-4)
        assert np.array_equal(p2p[lo:hi], rp2p) and np.array_equal(m2pc[lo:hi], rm2p)


@pytest.mark.gpu
def test_the_deepest_tree_the_stack_holds(hip):
    """a chain of 21 levels (node 0 of each level internal, 7 leaves beside it; M = 169) with every node opened: the
    stack of the depth-first walk peaks at 7 * 20 + 8 = 148 of its 160 entries.  CSTONE_OK, the direct sum, n_src - 1
    P2P per target"""
    tr = build_tree(chain_desc(21, 2))
    assert tr["M"] == 169
    rng = np.random.default_rng(13)
    x, y, z, m = place_sources(tr, rng)
    ns = tr["n_src"]
    ctr = centers_of(tr, x, y, z, m, lambda n: HUGE_MAC)
    d = upload(hip, tr, x, y, z, m, ctr)
    groups = list(range(0, ns, 64)) + [ns]
    eps2 = 1e-6
    rc, a, phi, p2p, m2pc = raw_gravity(hip, d, upsweep(hip, d), 0, ns, groups, 2, 1.0, eps2)
    assert rc == 0
    assert (p2p == ns - 1).all() and (m2pc == 0).all()
    ra, rphi = direct_sum(x, y, z, m, np.arange(ns), eps2=eps2)
    assert rel_err(a, ra).max() <= 1e-10 and (np.abs(phi - rphi) / np.abs(rphi)).max() <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2])
def test_one_and_two_particles(hip, n):
    tr = build_tree(n)
    x, y, z = np.array([[0.2, 0.3, 0.4], [0.7, 0.1, 0.5]][:n]).T
    m = np.array([1.5, 0.5][:n])
    ctr = centers_of(tr, x, y, z, m, lambda k: HUGE_MAC)
    d = upload(hip, tr, x, y, z, m, ctr)
    rc, a, phi, p2p, m2pc = raw_gravity(hip, d, upsweep(hip, d), 0, n, [0, n], 2, 2.0, 0.0)
    assert rc == 0 and (p2p == n - 1).all() and (m2pc == 0).all()
    ra, rphi = direct_sum(x, y, z, m, np.arange(n), G=2.0)
    if n == 1:
        assert (a == 0).all() and (phi == 0).all()
    assert np.allclose(a, ra, rtol=1e-14, atol=0) and np.allclose(phi, rphi, rtol=1e-14, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("rb,mb", [(64, 64), (64, 32), (32, 32), (32, 64)])
def test_upsweep_of_a_hand_built_tree(hip, rb, mb):
    """M and Q of every node against the direct formula about its centre, every (coordinates, masses) instantiation;
    the tolerances of test_upsweep_multipoles_equal_the_direct_formula"""
    tr = build_tree(three_level_desc())
    x, y, z, m = place_sources(tr, np.random.default_rng(14))
    rdt, mdt = (np.float64 if rb == 64 else np.float32), (np.float64 if mb == 64 else np.float32)
    xr, yr, zr = [a.astype(rdt).astype(np.float64) for a in (x, y, z)]
    mr = m.astype(mdt).astype(np.float64)
    ctr = centers_of(tr, xr, yr, zr, mr, lambda n: 1.0).astype(rdt).astype(np.float64)
    d = upload(hip, tr, xr, yr, zr, mr, ctr, rb, mb)
    got = upsweep(hip, d).cpu().numpy().astype(np.float64)
    want = direct_multipoles(tr, xr, yr, zr, mr, ctr)
    tol = 1e-10 if rb == 64 else 3e-4
    worst = 0.0
    for n in range(tr["M"]):
        assert abs(got[n, 0] - want[n, 0]) <= tol * want[n, 0], n
        if want[n, 0] == 0:
            assert (got[n] == 0).all()
            continue
        # (a node of one particle has Q = 0 about its centre: M edge^2 / 1000 as the floor of the scale)
        scale = max(np.abs(want[n, 1:7]).max(), 1e-3 * want[n, 0] * cube_of(tr["paths"][n])[1] ** 2)
        err = np.abs(got[n, 1:7] - want[n, 1:7]).max() / scale
        worst = max(worst, err)
        assert got[n, 7] == 0
    print(f"hand-built upsweep rb={rb} mb={mb}: worst relative |dQ| {worst:.1e}")
    assert worst <= tol


# ---------------------------------------------------------------------------------------------------------------------
# GPU: through the Domain
# ---------------------------------------------------------------------------------------------------------------------
def check_against_restatement(hip, s, xd, yd, zd, md, groups, rb, n_groups=40, seed=1, G=0.7, eps2=1e-6, picks=()):
    """counts of sampled groups (and of the groups `picks`) equal to the restatement's exactly, a / phi to its
    tolerance (test_gravity's)"""
    a, phi, p2p, m2pc = gpu_gravity(hip, s, xd, yd, zd, md, groups, order=2, G=G, eps2=eps2)
    g = groups.cpu().numpy().astype(np.int64)
    assert g[0] == 0 and g[-1] == s["view"].end_index
    tol = 1e-10 if rb == 64 else 1e-4
    rng = np.random.default_rng(seed)
    worst = 0.0
    for k in np.union1d(rng.choice(g.size - 1, min(n_groups, g.size - 1), replace=False), np.asarray(picks, int)):
        ra, rphi, rp2p, rm2p = walk_reference(s, g[k], g[k + 1], 2, G=G, eps2=eps2)
        sl = slice(g[k], g[k + 1])
        assert np.array_equal(p2p[sl], rp2p) and np.array_equal(m2pc[sl], rm2p), k
        worst = max(worst, rel_err(a[sl], ra).max(), (np.abs(phi[sl] - rphi) / np.abs(rphi)).max())
    assert worst <= tol, worst
    return a, phi, p2p, m2pc


def check_against_direct_sum(s, a, phi, n_tg, seed, G=1.0, eps2=0.0, what=""):
    """quadrupole accuracy of a theta = 0.5 walk: the bounds of test_accuracy_against_the_direct_sum"""
    n = s["x"].size
    tg = np.random.default_rng(seed).choice(n, min(n, n_tg), replace=False)
    ra, rphi = direct_sum(s["x"], s["y"], s["z"], s["m"], tg, G=G, eps2=eps2)
    e = rel_err(a[tg], ra)
    ep = np.abs(phi[tg] - rphi) / np.abs(rphi)
    print(f"{what}: |da| median {np.median(e):.1e} p99 {np.percentile(e, 99):.1e}; "
          f"|dphi| median {np.median(ep):.1e} p99 {np.percentile(ep, 99):.1e}")
    assert np.median(e) <= 1e-3 and np.percentile(e, 99) <= 1e-2
    assert np.median(ep) <= 1e-3 and np.percentile(ep, 99) <= 1e-2


def clump_cloud(n, seed):
    """the clustered cloud and 600 particles within 2e-5 of one point: with 32-bit keys (leaves no smaller than 2^-10
    of the box) at most 8 bottom-level leaves hold them, one of them more than 64"""
    x, y, z, m = clustered_cloud(n, seed)
    rng = np.random.default_rng(seed + 1)
    c = rng.uniform(-1e-5, 1e-5, (600, 3)) + [0.31, 0.62, 0.47]
    return (np.concatenate([x, c[:, 0]]), np.concatenate([y, c[:, 1]]), np.concatenate([z, c[:, 2]]),
            np.concatenate([m, np.full(600, m.mean())]))


@pytest.mark.gpu
@pytest.mark.parametrize("rb,kb,curve,bucket_focus,clump", [
    (64, 32, "hilbert", 16, False), (32, 32, "hilbert", 16, False), (64, 64, "morton", 16, False),
    (64, 32, "morton", 16, False), (64, 32, "hilbert", 16, True), (64, 64, "hilbert", 128, False),
    (32, 64, "hilbert", 300, False)])
def test_walk_of_every_key_width_curve_and_bucket(hip, rb, kb, curve, bucket_focus, clump):
    """the restatement's counts exactly and the direct sum's accuracy for the trees of 32-bit keys, the Morton curve,
    bottom-level leaves over the bucket and focus buckets of 128 and 300 (leaves of several 64-particle passes)"""
    import cstone_amd

    x, y, z, m = clump_cloud(30000, 16) if clump else clustered_cloud(30000, 16)
    cv = cstone_amd.HILBERT if curve == "hilbert" else cstone_amd.MORTON
    dom, xd, yd, zd, md = grav_domain(hip, x, y, z, m, rb, rb, theta=0.5, kb=kb, bucket_focus=bucket_focus, curve=cv)
    s = tree_state(hip, dom, xd, yd, zd, md, kb=kb)
    biggest = np.diff(s["layout"]).max()
    if clump or bucket_focus > 64:
        assert biggest > 64, biggest  # (clump: a bottom-level leaf the bucket cannot split)
    groups = groups_of(hip, s, xd, yd, zd)
    check_against_restatement(hip, s, xd, yd, zd, md, groups, rb)
    a, phi = gpu_gravity(hip, s, xd, yd, zd, md, groups, order=2, counts=False)
    check_against_direct_sum(s, a, phi, 1024, 3, what=f"rb={rb} kb={kb} {curve} bucket {bucket_focus} clump={clump}"
                                                       f" (largest leaf {biggest})")


# Worst |da| / (G sum_j m_j / r_ij^2) of the f32 all-opened walk on the MI355X 5.8e-6, relative |dphi| 8.6e-6.
@pytest.mark.gpu
def test_opening_everything_in_f32_is_the_direct_sum(hip):
    """float32 with every node opened: the direct sum, the force error normalised by the size of its terms (the f32 sum
    cancels near the centre of a blob), phi relative"""
    x, y, z, m = clustered_cloud(20000, 13)
    dom, xd, yd, zd, md = grav_domain(hip, x, y, z, m, 32, 32, theta=1e-6, bucket_focus=32)
    s = tree_state(hip, dom, xd, yd, zd, md)
    groups = groups_of(hip, s, xd, yd, zd)
    eps2 = 1e-4
    a, phi, p2p, m2pc = gpu_gravity(hip, s, xd, yd, zd, md, groups, eps2=eps2)
    n = x.size
    assert (m2pc == 0).all() and (p2p == n - 1).all()
    tg = np.random.default_rng(2).choice(n, 1024, replace=False)
    ra, rphi = direct_sum(s["x"], s["y"], s["z"], s["m"], tg, eps2=eps2)
    scale = force_scale(s["x"], s["y"], s["z"], s["m"], n, tg, eps2)
    ea = (np.linalg.norm(a[tg] - ra, axis=1) / scale).max()
    ep = (np.abs(phi[tg] - rphi) / np.abs(rphi)).max()
    print(f"f32 all opened: worst |da| / sum m/r^2 {ea:.1e}, relative |dphi| {ep:.1e}")
    assert ea <= 3e-5 and ep <= 3e-5


@pytest.mark.gpu
def test_massless_leaves_are_skipped_and_still_targets(hip):
    """a blob of massless particles in the void between the massive ones: set_mac gives its leaves macSq = 0, the walk
    skips them as sources and gives their particles the force of the others"""
    x, y, z, m = clustered_cloud(20000, 17)
    rng = np.random.default_rng(18)
    blob = rng.normal(0, 0.01, (2000, 3)) + 0.5
    x, y, z = [np.concatenate([a, blob[:, k]]) for k, a in enumerate((x, y, z))]
    m = np.concatenate([m, np.zeros(2000)])
    dom, xd, yd, zd, md = grav_domain(hip, x, y, z, m, theta=0.5, bucket_focus=16)
    s = tree_state(hip, dom, xd, yd, zd, md)
    leaf_nodes = s["leaf_to_internal"][s["M"] - s["L"]:]
    lm = np.array([s["m"][s["layout"][k]:s["layout"][k + 1]].sum() for k in range(s["L"])])
    nonempty = np.diff(s["layout"]) > 0
    massless = leaf_nodes[(lm == 0) & nonempty]
    assert massless.size > 0 and (s["centers"][massless, 3] == 0).all()
    groups = groups_of(hip, s, xd, yd, zd)
    in_blob = np.nonzero(s["m"] == 0)[0]
    g = groups.cpu().numpy()
    blob_groups = np.nonzero(s["m"][g[:-1]] == 0)[0]
    a, phi, _, _ = check_against_restatement(hip, s, xd, yd, zd, md, groups, 64, picks=blob_groups[::4])
    assert np.isfinite(a).all() and np.isfinite(phi).all()
    tg = np.random.default_rng(19).choice(in_blob, 256, replace=False)
    a2, phi2 = gpu_gravity(hip, s, xd, yd, zd, md, groups, counts=False)
    ra, rphi = direct_sum(s["x"], s["y"], s["z"], s["m"], tg)
    # (the blobs around the void pull its particles almost evenly: |da| normalised by the size of the terms)
    e = np.linalg.norm(a2[tg] - ra, axis=1) / force_scale(s["x"], s["y"], s["z"], s["m"], s["x"].size, tg)
    ep = np.abs(phi2[tg] - rphi) / np.abs(rphi)
    print(f"massless blob: {massless.size} massless leaves; |da| / sum m/r^2 median {np.median(e):.1e} max "
          f"{e.max():.1e}; |dphi| max {ep.max():.1e}")
    assert np.median(e) <= 1e-3 and e.max() <= 1e-2 and ep.max() <= 1e-3


@pytest.mark.gpu
def test_gravity_after_a_second_sync_and_after_recentring(hip):
    """sync_grav, gravity, drift, sync_grav, gravity: the second result is compute_gravity on groups computed afresh
    from the second sync, bit for bit.  Then drift without a sync and update_expansion_centers: Domain.gravity is
    compute_gravity with the kept groups and the new centres, whose counts equal the restatement's"""
    import torch

    x, y, z, m = clustered_cloud(30000, 20)
    dom, xd, yd, zd, md = grav_domain(hip, x, y, z, m, theta=0.5, bucket_focus=16)
    dom.gravity(xd, yd, zd, md)
    rng = np.random.default_rng(21)
    n = xd.numel()
    for a in (xd, yd, zd):
        a += torch.from_numpy(rng.normal(0, 0.01, n)).cuda()
    keys = torch.zeros(n, dtype=torch.int64, device="cuda")
    h = torch.full((n,), 0.01, dtype=xd.dtype, device="cuda")
    keys, xd, yd, zd, _, md, _, _ = dom.sync_grav(keys, xd.clone(), yd.clone(), zd.clone(), h, md.clone(),
                                                  [torch.empty_like(xd) for _ in range(3)])
    got = dom.gravity(xd, yd, zd, md, G=1.5)
    s = tree_state(hip, dom, xd, yd, zd, md)
    groups = groups_of(hip, s, xd, yd, zd)
    a, phi = gpu_gravity(hip, s, xd, yd, zd, md, groups, G=1.5, counts=False)
    assert np.array_equal(np.stack([t.cpu().numpy() for t in got[:3]], 1), a)
    assert np.array_equal(got[3].cpu().numpy(), phi)
    check_against_direct_sum(s, a, phi, 1024, 22, G=1.5, what="after the second sync_grav")
    # drift again, no sync: the groups stay, the centres follow the particles
    for t in (xd, yd, zd):
        t += torch.from_numpy(rng.normal(0, 5e-4, n)).cuda()  # (well inside a leaf: the MAC still holds)
    dom.update_expansion_centers(xd, yd, zd, md)
    got = dom.gravity(xd, yd, zd, md, G=1.5)
    s2 = tree_state(hip, dom, xd, yd, zd, md)
    assert not np.array_equal(s2["centers"], s["centers"])
    a, phi = gpu_gravity(hip, s2, xd, yd, zd, md, groups, G=1.5, counts=False)
    assert np.array_equal(np.stack([t.cpu().numpy() for t in got[:3]], 1), a)
    assert np.array_equal(got[3].cpu().numpy(), phi)
    check_against_restatement(hip, s2, xd, yd, zd, md, groups, 64, G=1.5, eps2=0.0)
    check_against_direct_sum(s2, a, phi, 1024, 22, G=1.5, what="after update_expansion_centers")


@pytest.mark.gpu
def test_f32_coordinates_with_f64_masses(hip):
    """(f32, f64) through the context API on an f32 domain's tree: both kernels convert the mass to the coordinates'
    type before use, so with masses that are floats widened to double the result is the (f32, f32) one bit for bit"""
    x, y, z, m = clustered_cloud(30000, 23)
    dom, xd, yd, zd, md = grav_domain(hip, x, y, z, m, 32, 32, theta=0.5, bucket_focus=16)
    s = tree_state(hip, dom, xd, yd, zd, md)
    d = s["dev"]
    mp64 = hip.upsweep_multipoles(xd, yd, zd, md.double(), d["lti_leaves"], d["layout"], s["level_range"],
                                  d["child_offsets"], d["centers"])
    hip.sync()
    assert torch_equal(mp64, d["multipoles"])
    groups = groups_of(hip, s, xd, yd, zd)
    a32, phi32, p32, m32 = gpu_gravity(hip, s, xd, yd, zd, md, groups)
    a64, phi64, p64, m64 = gpu_gravity(hip, s, xd, yd, zd, md.double(), groups)
    assert np.array_equal(a32, a64) and np.array_equal(phi32, phi64)
    assert np.array_equal(p32, p64) and np.array_equal(m32, m64)
    check_against_direct_sum(s, a64, phi64, 1024, 24, what="f32 coordinates, f64 masses")


def torch_equal(a, b):
    return bool((a == b).all().item())


@pytest.mark.gpu
@pytest.mark.parametrize("theta", [1e-6, 0.5])
def test_coincident_particles(hip, theta):
    """every position twice: a coincident pair adds no force and -G m / eps to phi (the direct sum, which has the
    same softening).  (theta = 0.5: the softened M2P is not the expansion of the softened potential, so the errors are
    about three times those without softening, still within the bounds)"""
    rng = np.random.default_rng(25)
    x, y, z, m = clustered_cloud(6000, 25)
    x, y, z = [np.concatenate([a, a]) for a in (x, y, z)]
    m = np.concatenate([m, rng.uniform(0.5, 2.0, m.size) / m.size])
    dom, xd, yd, zd, md = grav_domain(hip, x, y, z, m, theta=theta, bucket_focus=16)
    s = tree_state(hip, dom, xd, yd, zd, md)
    groups = groups_of(hip, s, xd, yd, zd)
    eps2 = 1e-4
    a, phi, p2p, m2pc = gpu_gravity(hip, s, xd, yd, zd, md, groups, G=1.0, eps2=eps2)
    assert np.isfinite(a).all() and np.isfinite(phi).all()
    if theta < 1e-3:
        n = s["x"].size
        assert (p2p == n - 1).all() and (m2pc == 0).all()
        tg = np.random.default_rng(26).choice(n, 1024, replace=False)
        ra, rphi = direct_sum(s["x"], s["y"], s["z"], s["m"], tg, eps2=eps2)
        assert rel_err(a[tg], ra).max() <= 1e-10 and (np.abs(phi[tg] - rphi) / np.abs(rphi)).max() <= 1e-10
    else:
        check_against_restatement(hip, s, xd, yd, zd, md, groups, 64, G=1.0, eps2=eps2)
        check_against_direct_sum(s, a, phi, 1024, 26, eps2=eps2, what="coincident pairs")
