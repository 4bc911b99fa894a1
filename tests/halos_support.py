"""Builders and the plain references of tests/test_halos.py (host side only, numpy and plain Python).

Everything here is integer geometry once a radius has become a cell count, and none of it shares code with the walk of
csrc/halos.hip or with the oracle's:

* decode_keys: Morton is bit de-interleaving; Hilbert is the decode recurrence restated as one table row per octal digit
  (which axes rotate, which axes flip, which bits are appended).  check_decoder pins both against oracle.compute_sfc_keys.
* Tree: every node of a cornerstone tree as an integer cube [lo, lo + edge)^3.
* dilated_boxes: the halo box of a leaf, per axis in the real type T of the call:
      inv = T(1) / (T(hi) - T(lo));  delta = min(uint(ceil(T(radius) * inv * T(2^L))), 2^L - 1)
      a = c - delta, b = c + edge + delta, clamped to [0, R] on a non-periodic axis (boundary type 0 or 2)
  numpy does not fuse the products and the multiplication by 2^L is exact, so the model is bit-exact.  It holds while
  radius / edge length < 2^(32 - L) (2048 for 64-bit keys, 4194304 for 32-bit keys): at or above that the conversion of
  the ceiling to unsigned is undefined in the reference too, and no shape here goes there.
* overlap_table: per axis two intervals overlap directly or after one shift by +-R (the ring rule), for every
  (target, cube) pair by broadcasting.
* brute_find_halos / brute_boxes / brute_overlaps / model_halo_radii: what the five entry points must return.
* wave_peak / dfs_peak: the wave walk (pop <= 8, push <= 64 per step) and the one-thread walk restated over the linked
  octree; they return stack heights and are used only to assert the premises of the shapes."""
import numpy as np

from helpers import Box, OctreeMaker, end_key, key_dtype, max_level, random_cloud, real_dtype
from oracle.oracle import HILBERT, MORTON

ANISO = [-1.3, 2.1, 0.2, 0.9, -5, 7]  # BOXES[1] of test_gpu_parity.py: x 3.4, y 0.7, z 12 long
BCS = {"000": (0, 0, 0), "111": (1, 1, 1), "100": (1, 0, 0), "010": (0, 1, 0), "012": (0, 1, 2), "221": (2, 2, 1)}
LENGTHS = (1, 63, 64, 65, 255, 256, 257)  # the edges of a wave and of a workgroup of four waves


# ---- keys -> integer cubes -------------------------------------------------------------------------------------------

def _compact(key, shift, levels):
    """every third bit of key, starting at bit `shift`"""
    out = np.zeros(key.shape, dtype=np.int64)
    for i in range(levels):
        out |= ((key >> np.uint64(3 * i + shift)) & np.uint64(1)).astype(np.int64) << i
    return out


# per octal digit xyz of a Hilbert key: how the point built from the lower digits is permuted (0 keep, 1 (x,y,z) <-
# (z,x,y), 2 swap x and z), which of its axes are mirrored, and the bits appended on top
_HILBERT_DIGIT = {
    0: (2, (0, 0, 0), (0, 0, 0)), 1: (1, (0, 0, 0), (0, 0, 1)), 2: (1, (0, 0, 0), (0, 1, 1)), 3: (0, (0, 1, 1), (0, 1, 0)),
    4: (0, (0, 1, 1), (1, 1, 0)), 5: (1, (1, 1, 0), (1, 1, 1)), 6: (1, (1, 1, 0), (1, 0, 1)), 7: (2, (1, 0, 1), (1, 0, 0)),
}


def decode_keys(keys, curve, kb):
    """[n, 3] integer coordinates of the finest cells the keys name"""
    L = max_level(kb)
    keys = np.asarray(keys).astype(np.uint64)
    if curve == MORTON:
        return np.stack([_compact(keys, 2, L), _compact(keys, 1, L), _compact(keys, 0, L)], axis=1)
    p = np.zeros((keys.size, 3), dtype=np.int64)
    for lvl in range(L):
        digit = ((keys >> np.uint64(3 * lvl)) & np.uint64(7)).astype(np.int64)
        perm = np.array([_HILBERT_DIGIT[d][0] for d in range(8)])[digit]
        flip = np.array([_HILBERT_DIGIT[d][1] for d in range(8)])[digit]
        bits = np.array([_HILBERT_DIGIT[d][2] for d in range(8)])[digit]
        rot, swp = (perm == 1)[:, None], (perm == 2)[:, None]
        p = np.where(rot, p[:, [2, 0, 1]], np.where(swp, p[:, [2, 1, 0]], p))
        p = p ^ (flip * ((1 << lvl) - 1))
        p = p | (bits << lvl)
    return p


def key_levels(leaves, kb):
    span = np.diff(leaves.astype(np.uint64)).astype(np.uint64)
    lg = np.array([int(s).bit_length() - 1 for s in span])
    assert (lg % 3 == 0).all() and all(1 << int(g) == int(s) for g, s in zip(lg, span))
    return max_level(kb) - lg // 3


def check_decoder(oracle, keys, levels, curve, kb):
    """the decoder against the oracle's ENCODER: the cell a key decodes to encodes back to that key, and the low corner
    of the level's cube around it encodes to a key of the same node (for Morton: to the node's start key itself).
    Box([0, 1]) in f64: i / 2^L and the encoder's i / 2^L * 2^L are exact"""
    L = max_level(kb)
    keys = np.asarray(keys).astype(key_dtype(kb))
    cell = decode_keys(keys, curve, kb)
    assert cell.min() >= 0 and cell.max() < (1 << L)
    back = oracle.compute_sfc_keys(curve, kb, *[np.ascontiguousarray(cell[:, d] / float(1 << L)) for d in range(3)],
                                   Box([0, 1]))
    assert np.array_equal(back, keys)
    edge = np.int64(1) << (L - np.asarray(levels))
    corner = cell & ~(edge - 1)[:, None]
    low = oracle.compute_sfc_keys(curve, kb, *[np.ascontiguousarray(corner[:, d] / float(1 << L)) for d in range(3)],
                                  Box([0, 1]))
    span = (np.uint64(1) << (3 * (L - np.asarray(levels))).astype(np.uint64)).astype(np.uint64)
    assert np.array_equal(low.astype(np.uint64) & ~(span - np.uint64(1)), keys.astype(np.uint64))
    if curve == MORTON:
        assert np.array_equal(low, keys)


class Tree:
    """a cornerstone leaf array with its linked octree (the oracle's) and the integer cube of every leaf and node"""

    def __init__(self, oracle, leaves, curve):
        self.kb = leaves.dtype.itemsize * 8
        self.curve, self.leaves = curve, leaves
        self.L = max_level(self.kb)
        self.R = 1 << self.L
        self.nl = leaves.size - 1
        assert int(leaves[0]) == 0 and int(leaves[-1]) == end_key(self.kb)
        self.o = oracle.build_octree(leaves)
        self.level = key_levels(leaves, self.kb)
        check_decoder(oracle, leaves[:-1], self.level, curve, self.kb)
        self.edge = np.int64(1) << (self.L - self.level)
        self.corner = decode_keys(leaves[:-1], curve, self.kb) & ~(self.edge - 1)[:, None]
        # nodes of the linked octree: prefix = 1 followed by 3 * level key bits
        pre = [int(p) for p in self.o["prefixes"]]
        self.node_level = np.array([(p.bit_length() - 1) // 3 for p in pre])
        start = [(p - (1 << (3 * l))) << (3 * (self.L - l)) for p, l in zip(pre, self.node_level.tolist())]
        self.node_start = np.array(start, dtype=np.uint64)
        self.node_span = np.array([1 << (3 * (self.L - l)) for l in self.node_level.tolist()], dtype=np.uint64)
        check_decoder(oracle, self.node_start, self.node_level, curve, self.kb)
        self.node_edge = np.int64(1) << (self.L - self.node_level)
        self.node_corner = decode_keys(self.node_start, curve, self.kb) & ~(self.node_edge - 1)[:, None]
        self.child = self.o["child_offsets"][:self.o["num_nodes"]].astype(np.int64)


def raw_delta(radii, box, rb, L):
    """ceil(T(radius) * inv * T(2^L)) per leaf and axis, before the clamp at 2^L - 1, as integers"""
    T = real_dtype(rb)
    lim = box.lim.astype(T)
    inv = T(1) / (lim[1::2] - lim[0::2])
    assert inv.dtype == T
    x = np.asarray(radii, dtype=np.float32).astype(T)[:, None] * inv[None, :]
    x = np.ceil(x * T(1 << L))
    assert x.dtype == T and x.max() < 2.0 ** 32  # the conversion to unsigned is defined
    return x.astype(np.int64)


def dilated_boxes(tree, radii, box, rb):
    """(lo, hi), each [num_leaves, 3]"""
    delta = np.minimum(raw_delta(radii, box, rb, tree.L), tree.R - 1)
    lo, hi = tree.corner - delta, tree.corner + tree.edge[:, None] + delta
    open_axis = np.array([int(b) != 1 for b in box.bc])
    lo = np.where(open_axis, np.clip(lo, 0, tree.R), lo)
    hi = np.where(open_axis, np.clip(hi, 0, tree.R), hi)
    return lo, hi


def overlap_table(R, a, b, c, d):
    """[len(c), len(a)]: cube [a, b) overlaps target [c, d) on all three axes under the ring rule"""
    out = np.ones((c.shape[0], a.shape[0]), dtype=bool)
    for x in range(3):
        ax, bx, cx, dx = a[None, :, x], b[None, :, x], c[:, None, x], d[:, None, x]
        direct = (bx > cx) & (dx > ax)
        mine_up = (bx + R > cx) & (dx > ax + R)
        other_up = (bx > cx + R) & (dx + R > ax)
        out &= direct | mine_up | other_up
    return out


class Halo:
    """one tree under one box, real type and radii array: the targets' boxes and the (target, leaf) overlap table"""

    def __init__(self, tree, radii, box, rb, targets=None):
        self.tree, self.radii, self.box, self.rb = tree, np.ascontiguousarray(radii, dtype=np.float32), box, rb
        self.lo, self.hi = dilated_boxes(tree, self.radii, box, rb)
        self.t0, self.t1 = (0, tree.nl) if targets is None else targets  # the targets the table is built for
        self._rows, self._ov = slice(self.t0, self.t1), None

    @property
    def ov(self):
        if self._ov is None:
            t = self.tree
            self._ov = overlap_table(t.R, t.corner, t.corner + t.edge[:, None], self.lo[self._rows], self.hi[self._rows])
        return self._ov

    def brute_find_halos(self, first, last):
        assert self.t0 <= first and last <= self.t1
        flags = self.ov[first - self.t0:last - self.t0].any(0).astype(np.int32)
        flags[first:last] = 0
        return flags

    def brute_boxes(self, first, last):
        """(plain, foreign): the eight columns of halo_boxes and of halo_boxes_foreign.  Column 6 of plain is the
        enclosing-node rule stated on the leaves: the smallest octree cube around a box that stays inside [0, R]^3
        consists of whole leaves or lies inside one, so its key range is inside the own range exactly if every leaf that
        meets it is; a box that leaves [0, R]^3 is inside only the full tree.  Column 6 of foreign: some leaf outside
        the range overlaps the box"""
        t = self.tree
        lo, hi = self.lo[first:last], self.hi[first:last]
        plain = np.zeros((last - first, 8), dtype=np.int32)
        plain[:, 0:6:2], plain[:, 1:6:2] = lo, hi
        foreign = plain.copy()
        wraps = (lo.min(1) < 0) | (hi.max(1) > t.R)
        diff = (np.clip(lo, 0, t.R - 1) ^ np.clip(hi - 1, 0, t.R - 1)).max(1)
        edge = np.int64(1) << np.array([int(v).bit_length() for v in diff], dtype=np.int64)
        corner = np.clip(lo, 0, t.R - 1) & ~(edge - 1)[:, None]
        meets = np.ones((last - first, t.nl), dtype=bool)
        for x in range(3):
            leaf_lo, leaf_hi = t.corner[None, :, x], (t.corner[:, x] + t.edge)[None, :]
            meets &= (leaf_hi > corner[:, None, x]) & ((corner[:, x] + edge)[:, None] > leaf_lo)
        outside = np.ones(t.nl, dtype=bool)
        outside[first:last] = False
        inside = np.where(wraps, first == 0 and last == t.nl, ~(meets & outside[None, :]).any(1))
        plain[:, 6] = ~inside
        foreign[:, 6] = (self.ov[first - self.t0:last - self.t0] & outside[None, :]).any(1)
        return plain, foreign


def brute_overlaps(tree, records, first, last):
    """uint32 words: 1 << (rec[7] & 31) OR-ed into leaf l of [first, last) for every record with rec[6] != 0 whose box
    overlaps the leaf's cube; 0 outside the range"""
    rec = np.asarray(records, dtype=np.int64).reshape(-1, 8)
    words = np.zeros(tree.nl, dtype=np.uint32)
    if rec.shape[0] == 0 or first == last:
        return words
    s = slice(first, last)
    ov = overlap_table(tree.R, tree.corner[s], (tree.corner + tree.edge[:, None])[s], rec[:, 0:6:2], rec[:, 1:6:2])
    for j in np.flatnonzero(rec[:, 6] != 0):
        words[s][ov[j]] |= np.uint32(1 << (int(rec[j, 7]) & 31))
    return words


def model_halo_radii(h, layout, first, last, nl, ext):
    """float32(max(h of the leaf) * Th(2) * Th(ext)) in the type Th of h, 0 for an empty leaf, 0 outside [first, last);
    layout = last - first + 1 offsets into h"""
    Th = h.dtype.type
    out = np.zeros(nl, dtype=np.float32)
    for i in range(first, last):
        a, b = int(layout[i - first]), int(layout[i - first + 1])
        if b > a:
            out[i] = np.float32(h[a:b].max() * Th(2) * Th(np.float32(ext)))
    return out


# ---- the walks, restated for their stack heights ---------------------------------------------------------------------

def node_interest(tree, lo, hi, first, last, serve):
    """go[node] for one target box: find mode skips the nodes inside the own key range, serve mode those outside it"""
    ov = overlap_table(tree.R, tree.node_corner, tree.node_corner + tree.node_edge[:, None], lo[None, :], hi[None, :])[0]
    lowest, highest = np.uint64(tree.leaves[first]), np.uint64(tree.leaves[last])
    start = tree.node_start
    end_le_highest = (start + (tree.node_span - np.uint64(1))) < highest  # end <= highest without overflowing 2^64
    if serve:
        mine = (start + (tree.node_span - np.uint64(1)) >= lowest) & (start < highest)
        return ov & mine
    return ov & ~((start >= lowest) & end_le_highest)


def wave_peak(tree, go):
    """peak height of the wave's stack: up to 8 nodes are popped from the top per step, their 64 children tested, the
    internal ones that are of interest pushed back"""
    if not go[0] or tree.child[0] == 0:
        return 0
    child, stack, peak = tree.child.tolist(), [0], 1
    while stack:
        take = min(len(stack), 8)
        popped = [stack.pop() for _ in range(take)]
        for par in popped:
            for c in range(child[par], child[par] + 8):
                if go[c] and child[c] != 0:
                    stack.append(c)
        peak = max(peak, len(stack))
    return peak


def dfs_peak(tree, go):
    """peak height of the one-thread walk's stack (the root occupies the first entry): what must stay below 128 for the
    reference's own code to run the shape"""
    if not go[0] or tree.child[0] == 0:
        return 0
    child, stack, peak, node = tree.child.tolist(), [0], 1, 0
    while True:
        for c in range(child[node], child[node] + 8):
            if go[c] and child[c] != 0:
                stack.append(c)
                peak = max(peak, len(stack))
        node = stack.pop()
        if node == 0:
            return peak


# ---- the shapes ------------------------------------------------------------------------------------------------------

def ranges_of(nl):
    """the wave and workgroup edges at the start, in the middle and at the end of the tree, all of it, nothing of it"""
    out = []
    for n in LENGTHS:
        if n <= nl:
            out += [(0, n), ((nl - n) // 2, (nl - n) // 2 + n), (nl - n, nl)]
    out += [(0, nl), (nl // 3, nl // 3)]
    return list(dict.fromkeys(out))


RADIUS_CLASSES = ("zero", "subcell", "face", "y04", "edge1", "edge4")


def aniso_radii(tree, box, kind, seed=11):
    """per leaf one of: 0; 0.3 of a finest cell of the shortest axis (a fraction of a cell on every axis); the distance
    to a face of the box along one axis, half a cell short, so that the ceiling ends the box exactly on the face;
    0.4 x the y length; 1 x and 4 x the longest length (both clamp).  kind "mix": all classes, "small": the first, second
    and fourth only (a range of leaves then flags a neighbourhood, not the whole tree)"""
    rng = np.random.default_rng(seed)
    ln = box.lim[1::2] - box.lim[0::2]
    cell = ln / tree.R
    classes = {"mix": (0, 1, 2, 3, 4, 5), "small": (0, 1, 3)}[kind]
    cls = np.array(classes)[rng.integers(0, len(classes), tree.nl)]
    axis, side = rng.integers(0, 3, tree.nl), rng.integers(0, 2, tree.nl)
    cells = np.where(side == 0, tree.corner[np.arange(tree.nl), axis],
                     tree.R - tree.corner[np.arange(tree.nl), axis] - tree.edge)
    face = np.maximum(cells - 0.5, 0.0) * cell[axis]
    table = np.stack([np.zeros(tree.nl), np.full(tree.nl, 0.3 * cell.min()), face, np.full(tree.nl, 0.4 * ln[1]),
                      np.full(tree.nl, ln.max()), np.full(tree.nl, 4 * ln.max())])
    return table[cls, np.arange(tree.nl)].astype(np.float32), cls


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def aniso_tree(oracle, kb, curve):
    """2000 clustered particles in the anisotropic box, bucket 8: about 1300 leaves"""
    def make():
        box = Box(ANISO)
        x, y, z = random_cloud(2000, box, 64, 5, "clustered")
        keys = np.sort(oracle.compute_sfc_keys(curve, kb, x, y, z, box))
        leaves, _ = oracle.compute_octree(keys, 8)
        return Tree(oracle, leaves, curve)
    return cached(("aniso", kb, curve), make)


def single_tree(oracle, kb, curve):
    return cached(("single", kb, curve),
                  lambda: Tree(oracle, np.array([0, end_key(kb)], dtype=key_dtype(kb)), curve))


def eight_tree(oracle, kb, curve):
    return cached(("eight", kb, curve), lambda: Tree(oracle, OctreeMaker(kb).divide().make(), curve))


DEEP_PATHS = {"corner": lambda L: [0] * L, "mixed": lambda L: [(3 * i + 5) % 8 for i in range(L)]}


def deep_tree(oracle, kb, curve, path):
    """refined along one key path down to the deepest level: 7 L + 1 leaves, the last eight of edge 1"""
    def make():
        L, m = max_level(kb), OctreeMaker(kb).divide()
        digits = DEEP_PATHS[path](L)
        for lvl in range(1, L):
            m.divide(*digits[:lvl])
        return Tree(oracle, m.make(), curve)
    return cached(("deep", kb, curve, path), make)


WIDE_LEVEL = 5


def wide_tree(oracle, kb, curve):
    """the uniform tree of WIDE_LEVEL levels (32768 leaves)"""
    def make():
        n = 8 ** WIDE_LEVEL
        span = end_key(kb) // n
        return Tree(oracle, (np.arange(n + 1, dtype=np.uint64) * np.uint64(span)).astype(key_dtype(kb)), curve)
    return cached(("wide", kb, curve), make)
