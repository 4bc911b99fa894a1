"""Builders and the plain models of tests/test_focus_walk.py (host side only, numpy and plain Python).

Nothing here shares code with csrc/focus.hip or with the oracle:

* encode_cells: the inverse of halos_support.decode_keys (Morton: bit interleaving; Hilbert: the decode table read
  backwards, one octal digit per level from the top), pinned by the round trip through decode_keys.
* mark_macs_model: the rule of markMacs (R/traversal/macs.hpp:195-269, R/traversal/boxoverlap.hpp:93-116) as a brute
  force over all (target, node) pairs in the real type T of the call:
      target cube   integer cube of focus node i; half = T(0.5) * (T(1) / 2^L) * len, centre = lo + T(hi + lo) * half,
                    size = T(hi - lo) * half
      skipped       the cube grown by one cell: outside [0, 2^L] on any axis -> skipped only if the focus is the whole
                    key range; else the smallest octree node around the keys of its low corner and of its high corner
                    minus one lies inside [focusStart, focusEnd)
      v(t, n)       node n not fully inside the focus; per axis dx = c_t - c_n; dx -= pbcLen * rint(dx * inv);
                    dx = |dx| - s_t; dx += |dx|; dx *= 0.5; r2 = dx0^2 + (dx1^2 + dx2^2); r2 < |centers[n][3]| and
                    level(n) <= maxSourceLevel(t)
      reach(t, n)   v(t, n) and reach(t, parent(n)), level by level; marks = initial, zeros become 1 where some target
                    that is not skipped reaches the node
  numpy does not fuse a product into a sum and the kernels are built with -ffp-contract=off, so the model is bit-exact.
  `variant` restates one wrong rule at a time; the tests use the variants only to show that their shapes can tell the
  rule from its neighbours (the premise of a case), never to judge a kernel.
* probe_centers: centres that make the set of walked targets visible in the marks: every node fails the MAC against
  every target (fourth entry huge), except one leaf per target, whose centre is the target's centre and whose radius is
  so small that only this target (distance 0) fails it.
* the per-node and per-leaf models of part 2, from the contracts in include/cstone_hip.h, with key arithmetic on Python
  ints."""
import ctypes as C

import numpy as np

import halos_support as hs
from helpers import end_key, key_dtype, max_level, real_dtype
from oracle.oracle import MORTON

HUGE = 1e30  # a squared radius no squared distance in any box here reaches, finite in f32


# ---- integer cells -> keys -------------------------------------------------------------------------------------------

_DIGIT_OF_BITS = np.zeros(8, dtype=np.int64)
for _d, (_perm, _flip, _bits) in hs._HILBERT_DIGIT.items():
    _DIGIT_OF_BITS[_bits[0] * 4 + _bits[1] * 2 + _bits[2]] = _d
_PERM = np.array([hs._HILBERT_DIGIT[d][0] for d in range(8)])
_FLIP = np.array([hs._HILBERT_DIGIT[d][1] for d in range(8)])


def encode_cells(cells, curve, kb):
    """uint64 keys of [n, 3] integer cells: decode_keys read backwards"""
    L = max_level(kb)
    p = np.array(cells, dtype=np.int64).reshape(-1, 3)
    assert p.size == 0 or (p.min() >= 0 and p.max() < (1 << L))
    keys =np.zeros(p.shape[0], dtype=np.uint64)
    if curve == MORTON:
        for i in range(L):
            for axis, shift in ((0, 2), (1, 1), (2, 0)):
                keys |= ((p[:, axis] >> i) & 1).astype(np.uint64) << np.uint64(3 * i + shift)
        return keys
    for lvl in range(L - 1, -1, -1):
        top = (p >> lvl) & 1
        digit = _DIGIT_OF_BITS[top[:, 0] * 4 + top[:, 1] * 2 + top[:, 2]]
        keys |= digit.astype(np.uint64) << np.uint64(3 * lvl)
        q = (p & ((1 << lvl) - 1)) ^ (_FLIP[digit] * ((1 << lvl) - 1))
        rot, swp = (_PERM[digit] == 1)[:, None], (_PERM[digit] == 2)[:, None]
        p = np.where(rot, q[:, [1, 2, 0]], np.where(swp, q[:, [2, 1, 0]], q))
    return keys


def check_encoder(curve, kb, seed=0):
    L = max_level(kb)
    cells = np.random.default_rng(seed).integers(0, 1 << L, (4000, 3))
    cells[:4] = [[0, 0, 0], [(1 << L) - 1] * 3, [0, (1 << L) - 1, 1], [1 << (L - 1), 0, (1 << (L - 1)) - 1]]
    assert np.array_equal(hs.decode_keys(encode_cells(cells, curve, kb), curve, kb), cells)


# ---- geometry --------------------------------------------------------------------------------------------------------

def parents_of(tree):
    par = np.zeros(tree.child.size, dtype=np.int64)
    for p in np.flatnonzero(tree.child):
        par[tree.child[p]:tree.child[p] + 8] = p
    return par


def center_and_size(lo, hi, box, rb, L):
    """centerAndSize (R/sfc/box.hpp:335-352) of integer cubes [lo, hi) in T"""
    T = real_dtype(rb)
    lim = box.lim.astype(T)
    half = T(0.5) * (T(1) / T(1 << L)) * (lim[1::2] - lim[0::2])
    assert half.dtype == T
    c = lim[0::2][None, :] + (hi + lo).astype(T) * half[None, :]
    s = (hi - lo).astype(T) * half[None, :]
    assert c.dtype == T and s.dtype == T
    return c, s


def node_geometry(tree, box, rb):
    return center_and_size(tree.node_corner, tree.node_corner + tree.node_edge[:, None], box, rb, tree.L)


def geo_spheres_model(tree, box, rb, inv_theta):
    """computeMinMacR2: (geometric centre, (2 max(size) invTheta)^2), invTheta a float"""
    T = real_dtype(rb)
    c, s = node_geometry(tree, box, rb)
    mac = (T(2) * s.max(axis=1)) * T(np.float32(inv_theta))
    out = np.concatenate([c, (mac * mac)[:, None]], axis=1)
    assert out.dtype == T
    return out


def set_mac_model(tree, box, rb, inv_theta, spheres):
    """computeVecMacR2 / setMac: (2 max(size) invTheta + |centre - geometric centre|)^2, 0 where the entry was 0"""
    T = real_dtype(rb)
    c, s = node_geometry(tree, box, rb)
    d = spheres[:, :3] - c
    dist = np.sqrt(d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]))
    mac = (T(2) * s.max(axis=1)) * T(np.float32(inv_theta)) + dist
    out = spheres.copy()
    out[:, 3] = np.where(spheres[:, 3] != 0, mac * mac, T(0))
    assert out.dtype == T
    return out


def target_cubes(focus_nodes, curve, kb):
    L = max_level(kb)
    if len(focus_nodes) < 2:
        return np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int64), np.zeros(0, np.int64)
    level = hs.key_levels(np.asarray(focus_nodes), kb)
    edge = np.int64(1) << (L - level)
    lo = hs.decode_keys(focus_nodes[:-1], curve, kb) & ~(edge - 1)[:, None]
    return lo, lo + edge[:, None], level


OUT_OF_GRID, ENVELOPE_INSIDE, ENVELOPE_OUTSIDE = 0, 1, 2


def contained_in(lo, hi, curve, kb, focus_start, focus_end, variant=None):
    """(skipped, branch) per target cube"""
    L = max_level(kb)
    R = 1 << L
    elo, ehi = lo - 1, hi + 1
    out = (elo.min(axis=1) < 0) | (ehi.max(axis=1) > R)
    whole = focus_start == 0 and focus_end == end_key(kb)
    top = ehi if variant == "ehi" else ehi - 1
    k0 = encode_cells(np.clip(elo, 0, R - 1), curve, kb)
    k1 = encode_cells(np.clip(top, 0, R - 1), curve, kb)
    skipped = np.zeros(lo.shape[0], dtype=bool)
    branch = np.zeros(lo.shape[0], dtype=np.int64)
    for i in range(lo.shape[0]):
        if out[i]:
            skipped[i] = True if variant == "outgrid_true" else whole
            branch[i] = OUT_OF_GRID
            continue
        a, b = int(k0[i]), int(k1[i])
        common = (3 * L - (a ^ b).bit_length()) // 3  # octal digits the two keys share from the top
        span = 1 << (3 * (L - common))
        start = a // span * span
        skipped[i] = start >= focus_start and start + span <= focus_end
        branch[i] = ENVELOPE_INSIDE if skipped[i] else ENVELOPE_OUTSIDE
    return skipped, branch


class MacModel:
    """mark_macs as a brute force.  marks, skipped, branch (per target), v and reach ([walked targets, nodes])"""

    def __init__(self, tree, centers, box, rb, focus_nodes, limit, initial=None, variant=None):
        T = real_dtype(rb)
        L, kb = tree.L, tree.kb
        centers = np.asarray(centers)
        assert centers.dtype == T and centers.shape == (tree.child.size, 4)
        fs, fe = int(focus_nodes[0]), int(focus_nodes[-1])
        lo, hi, level = target_cubes(focus_nodes, tree.curve, kb)
        self.level = level
        self.skipped, self.branch = contained_in(lo, hi, tree.curve, kb, fs, fe, variant)
        self.walked = np.flatnonzero(~self.skipped)
        tc, ts = center_and_size(lo[self.walked], hi[self.walked], box, rb, L)
        if limit:
            max_src = level[self.walked] - 1 if variant == "nofloor" else np.maximum(level[self.walked] - 1, 0)
        else:
            max_src = np.full(self.walked.size, L)
        start = tree.node_start
        last = start + (tree.node_span - np.uint64(1))  # inclusive end: no overflow
        in_focus = (start >= np.uint64(fs)) & (last < np.uint64(fe))
        lim = box.lim.astype(T)
        length = lim[1::2] - lim[0::2]
        inv = T(1) / length
        fold_types = (1, 2) if variant == "fold2" else ((1,) if variant != "nofold" else ())
        pbc = np.array([T(int(b) in fold_types) for b in box.bc], dtype=T) * length
        r2 = None
        for d in (2, 1, 0):
            dx = tc[:, None, d] - centers[None, :, d]
            dx = dx - pbc[d] * np.rint(dx * inv[d])
            dx = np.abs(dx)
            dx = dx - ts[:, None, d]
            dx = dx + np.abs(dx)
            dx = dx * T(0.5)
            sq = dx * dx
            r2 = sq if d == 2 else (r2 + sq if d == 1 else sq + r2)  # dx0^2 + (dx1^2 + dx2^2)
        assert r2.dtype == T
        mac = centers[:, 3] if variant == "nofabs" else np.abs(centers[:, 3])
        near = r2 <= mac[None, :] if variant == "le" else r2 < mac[None, :]
        lvl = tree.node_level[None, :]
        shallow = lvl < max_src[:, None] if variant == "lt_level" else lvl <= max_src[:, None]
        self.v = near & shallow & ~in_focus[None, :]
        par = parents_of(tree)
        self.reach = self.v.copy()
        for l in range(1, int(tree.node_level.max()) + 1):
            idx = np.flatnonzero(tree.node_level == l)
            self.reach[:, idx] = self.v[:, idx] & self.reach[:, par[idx]]
        self.initial = np.zeros(tree.child.size, np.int8) if initial is None else np.asarray(initial, np.int8)
        self.marks = self.initial.copy()
        self.marks[(self.initial == 0) & self.reach.any(axis=0)] = 1
        self.in_focus = in_focus

    def peak(self, tree):
        """the highest stack of the wave walk over the walked targets"""
        return max([hs.wave_peak(tree, self.v[i]) for i in range(self.walked.size)] + [0])


def probe_centers(tree, box, rb, focus_nodes, radius_of=lambda i: 1.0):
    """(centers, probe): every node fails the MAC against every target, except probe[i], a leaf outside the focus whose
    centre is the centre of target i and whose squared radius is radius_of(i) x a hundredth of the squared half edge of
    a finest cell on the shortest axis: only target i is closer than that (distance 0)"""
    T = real_dtype(rb)
    fs, fe = np.uint64(int(focus_nodes[0])), np.uint64(int(focus_nodes[-1]))
    lo, hi, _ = target_cubes(focus_nodes, tree.curve, tree.kb)
    tc, _ = center_and_size(lo, hi, box, rb, tree.L)
    c, _ = node_geometry(tree, box, rb)
    centers = np.concatenate([c, np.full((c.shape[0], 1), HUGE, dtype=T)], axis=1).astype(T)
    last = tree.node_start + (tree.node_span - np.uint64(1))
    outside = ~((tree.node_start >= fs) & (last < fe))
    leaves = np.flatnonzero((tree.child == 0) & outside)
    assert leaves.size >= tc.shape[0], (leaves.size, tc.shape[0])
    probe = leaves[:tc.shape[0]]
    cell = (box.lim[1::2] - box.lim[0::2]).min() / tree.R
    tiny = 0.01 * (0.5 * cell) ** 2
    centers[probe, :3] = tc
    centers[probe, 3] = np.array([radius_of(i) * tiny for i in range(probe.size)], dtype=T)
    return centers, probe


# ---- the per-node and per-leaf models (part 2) -----------------------------------------------------------------------

def node_keys(octree, kb):
    """(start, level, span) of every node as Python ints, from the placeholder-bit prefixes"""
    L = max_level(kb)
    out = []
    for p in octree["prefixes"].tolist():
        level = (int(p).bit_length() - 1) // 3
        start = (int(p) - (1 << (3 * level))) << (3 * (L - level))
        out.append((start, level, 1 << (3 * (L - level))))
    return out


def node_parents(octree):
    """parent of every node (parents[] holds one entry per group of eight siblings)"""
    nn = octree["num_nodes"]
    par = [0] * nn
    for i in range(1, nn):
        par[i] = int(octree["parents"][(i - 1) // 8])
    return par


def essential_model(octree, kb, counts, macs, fs, fe, bucket, variant=None):
    """rebalance_decision_essential: 0 when the parent's count fits the bucket, or the parent passed the MAC and its
    children's key range does not touch the focus; else 8 for a leaf above the deepest level with count > bucket that
    fails the MAC or starts in the focus; else 1"""
    L = max_level(kb)
    nk, par, child = node_keys(octree, kb), node_parents(octree), octree["child_offsets"]
    ops = np.ones(len(nk), dtype=np.int32)
    for i, (start, level, span) in enumerate(nk):
        if i > 0:
            p = par[i]
            g0, g1 = nk[p][0], nk[p][0] + nk[p][2]
            fringe = g1 > fs and fe > g0 and variant != "nofringe"
            if int(counts[p]) <= bucket or (macs[p] == 0 and not fringe):
                ops[i] = 0
                continue
        if child[i] == 0 and level < L and int(counts[i]) > bucket and (macs[i] != 0 or fs <= start < fe):
            ops[i] = 8
    return ops


def mac_refine_model(octree, kb, macs, first, last):
    L = max_level(kb)
    nk = node_keys(octree, kb)
    l2i = octree["leaf_to_internal"][octree["num_internal"]:]
    ops = np.ones(l2i.size, dtype=np.int32)
    for i, n in enumerate(l2i.tolist()):
        if not first <= i < last and nk[n][1] < L and macs[n] != 0:
            ops[i] = 8
    return ops


def protect_model(octree, kb, ops):
    """the sequential rule, in place and in node order like the reference's loop: a 0 takes the op of its closest
    ancestor with a non-zero op if both start at the same key, and stays 0 otherwise"""
    nk, par = node_keys(octree, kb), node_parents(octree)
    ops = [int(v) for v in ops]
    changes = 0
    for i in range(len(ops)):
        a = i
        while ops[a] == 0 and a != 0:
            a = par[a]
        new = ops[a] if (a == i or nk[a][0] == nk[i][0]) else 0
        changes += new != 1
        ops[i] = new
    return np.array(ops, dtype=np.int32), changes == 0


def enforce_model(keys, octree, kb, ops):
    """the reference's sequential loop over the keys (enforceKeySingle, R/focus/rebalance.hpp:199-250)"""
    L = max_level(kb)
    nk, par, child = node_keys(octree, kb), node_parents(octree), octree["child_offsets"]
    ops = [int(v) for v in ops]
    status = 0
    for key in [int(k) for k in keys]:
        if key == 0 or key == end_key(kb):
            continue
        tz = (key & -key).bit_length() - 1
        want_level = L - tz // 3
        node = 0
        while child[node] != 0 and not (nk[node][0] == key and nk[node][1] == want_level):
            digit = (key >> (3 * (L - nk[node][1] - 1))) & 7
            node = int(child[node]) + digit
        have_level = nk[node][1]
        there = nk[node][0] == key and have_level == want_level
        split = not there and have_level < L
        st = 0
        if (ops[node] == 0 or split) and node > 0:
            st = 1
            p = node
            while True:
                p = par[p]
                for s in range(int(child[p]), int(child[p]) + 8):
                    if ops[s] == 0:
                        ops[s] = 1
                if p == 0:
                    break
        if split:
            st = 3 if want_level - have_level > 1 else 2
            ops[node] = max(ops[node], 8)
        status = max(status, st)
    return np.array(ops, dtype=np.int32), status


def range_count_model(leaves, counts, leaves_focus, idx, preset):
    gl = [int(k) for k in leaves]
    at = {k: i for i, k in enumerate(gl)}
    out = preset.copy()
    for j in [int(v) for v in idx]:
        a, b = at[int(leaves_focus[j])], at[int(leaves_focus[j + 1])]
        out[j] = min(sum(int(c) for c in counts[a:b]), 0xFFFFFFFF)
    return out


def tile(a, b, kb):
    """the fewest aligned nodes tiling [a, b): greedily the biggest node that starts at a and ends at or before b"""
    out = []
    while a < b:
        size = end_key(kb)
        while a % size != 0 or a + size > b:
            size //= 8
        out.append(a)
        a += size
    return out


def source_centers_model(x, y, z, m, l2i, layout, num_nodes, Tf):
    """serial loop in Tf, particle order: centre = sum(|m| r) / sum(|m|), inv = 1 when the sum is 0"""
    out = np.zeros((num_nodes, 4), dtype=Tf)
    zero, one = Tf(0), Tf(1)
    for leaf, n in enumerate(l2i.tolist()):
        cx = cy = cz = cm = zero
        for i in range(int(layout[leaf]), int(layout[leaf + 1])):
            w = abs(Tf(m[i]))
            cx, cy, cz, cm = cx + w * Tf(x[i]), cy + w * Tf(y[i]), cz + w * Tf(z[i]), cm + w
        inv = one / cm if cm != zero else one
        out[n] = cx * inv, cy * inv, cz * inv, cm
    assert out.dtype == Tf
    return out


def upsweep_model(octree, centers, variant=None):
    """internal nodes bottom-up: the eight children combined with their |mass| in child order"""
    Tf = centers.dtype.type
    out = centers.copy()
    child = octree["child_offsets"]
    zero, one = Tf(0), Tf(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        for n in range(octree["num_nodes"] - 1, -1, -1):  # nodes are stored level by level: children behind parents
            if child[n] == 0:
                continue
            cx = cy = cz = cm = zero
            for k in range(int(child[n]), int(child[n]) + 8):
                w = abs(out[k, 3])
                cx, cy, cz, cm = cx + w * out[k, 0], cy + w * out[k, 1], cz + w * out[k, 2], cm + w
            inv = one / cm if (cm != zero or variant == "noguard") else one
            out[n] = cx * inv, cy * inv, cz * inv, cm
    return out


# ---- calling the ABI -------------------------------------------------------------------------------------------------

def cbox(box):
    import cstone_amd

    return cstone_amd.make_cbox(box.lim, box.bc)


def call_mark_macs(be, tree, centers, box, rb, focus_nodes, limit, initial):
    """markings after cstone_hip_mark_macs on backend `be`, and the return code of the sync behind it"""
    kb = tree.kb
    nn = tree.child.size
    pre = be.to_dev(tree.o["prefixes"])
    co = be.to_dev(tree.o["child_offsets"])
    ce = be.to_dev(np.ascontiguousarray(centers).reshape(-1))
    fn = be.to_dev(np.ascontiguousarray(focus_nodes, dtype=key_dtype(kb)))
    marks = be.to_dev(np.ascontiguousarray(initial, dtype=np.int8))
    cb = cbox(box)
    be.chk(be.lib.cstone_hip_mark_macs(be.ctx, C.c_int(tree.curve), C.c_int(kb), C.c_int(rb), be.ptr(pre), be.ptr(co),
                                       be.ptr(ce), C.byref(cb), be.ptr(fn), C.c_int(len(focus_nodes) - 1),
                                       C.c_int(int(limit)), be.ptr(marks)), "mark_macs")
    be.chk(be.lib.cstone_hip_ctx_sync(be.ctx), "ctx_sync")
    out = be.to_host(marks, np.int8)
    assert out.size == nn
    return out
