"""TEST INFRASTRUCTURE for tests/test_let_ops.py: the two backends every test body runs on, the trees the inputs are
built from, and the numpy models of the device operations of the locally essential tree.

Backends.  `cpu`: "device" memory is host memory, the C ABI is served by oracle/libcstone_cabi_oracle.so (the project's
CPU restatement behind include/cstone_hip.h, built on demand by oracle/Makefile).  `hip`: torch tensors on the GPU and
libcstone_hip.so.  Both offer lib, ctx, to_dev, to_host, ptr and sync, so a test body does not know which one it has.

Models.  Each one restates the CONTRACT of its entry -- the comment in include/cstone_hip.h and the reference lines cited
there (R = the reference's include/cstone) -- in integer numpy with np.searchsorted; none of them follows a kernel or
oracle/cabi_on_oracle.cpp.  The cpu leg checks a model against the CPU restatement before the hip leg lets it judge a
kernel."""
import ctypes as C
import os

import numpy as np

from oracle import oracle as orc

E_ARG = -1


# ----------------------------------------------------------------------------------------------------------------------
# backends
# ----------------------------------------------------------------------------------------------------------------------
class Buf:
    """a device allocation: raw bytes (numpy uint8 array | torch uint8 tensor) and how many of them are payload"""

    def __init__(self, raw, nbytes):
        self.raw, self.nbytes = raw, nbytes


class _Backend:
    def chk(self, rc, what):
        if rc != 0:
            msg = self.lib.cstone_hip_last_error(self.ctx)
            raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def last_error(self):
        msg = self.lib.cstone_hip_last_error(self.ctx)
        return msg.decode() if msg else ""

    def filled(self, n, dtype, value):
        return self.to_dev(np.full(n, value, dtype))

    def ptrs(self, bufs):
        """a host array of device pointers (const void* const*)"""
        return (C.c_void_p * len(bufs))(*[self.ptr(b).value for b in bufs])


class CpuBackend(_Backend):
    name = "cpu"
    # (CSTONE_CABI_ORACLE_LIB: the sanitizer build of `make -C oracle asan`)
    libpath = os.environ.get("CSTONE_CABI_ORACLE_LIB", os.path.join(orc.HERE, "libcstone_cabi_oracle.so"))

    def __init__(self):
        if not os.path.exists(self.libpath):
            orc.build("cabi")
        self.lib = C.CDLL(self.libpath)
        self.lib.cstone_hip_last_error.restype = C.c_char_p
        self.ctx = C.c_void_p()
        assert self.lib.cstone_hip_ctx_create(C.byref(self.ctx), 0, None, 0) == 0

    def to_dev(self, a):
        a = np.ascontiguousarray(a)
        raw = np.zeros(max(a.nbytes, 8), np.uint8)
        raw[:a.nbytes] = a.view(np.uint8).reshape(-1)
        return Buf(raw, a.nbytes)

    def to_host(self, b, dtype):
        return b.raw[:b.nbytes].copy().view(dtype)

    def ptr(self, b, byte_offset=0):
        return C.c_void_p(0) if b is None else C.c_void_p(b.raw.ctypes.data + byte_offset)

    def sync(self):
        pass


class HipBackend(_Backend):
    name = "hip"

    def __init__(self, context):
        """context: cstone_amd.Context (the `hip` fixture); its work is ordered on torch's current stream"""
        self.context = context
        self.lib, self.ctx = context.lib, context.h

    def to_dev(self, a):
        import torch

        a = np.ascontiguousarray(a)
        raw = np.zeros(max(a.nbytes, 8), np.uint8)
        raw[:a.nbytes] = a.view(np.uint8).reshape(-1)
        return Buf(torch.from_numpy(raw).cuda(), a.nbytes)

    def to_host(self, b, dtype):
        return b.raw.cpu().numpy()[:b.nbytes].copy().view(dtype)

    def ptr(self, b, byte_offset=0):
        return C.c_void_p(0) if b is None else C.c_void_p(b.raw.data_ptr() + byte_offset)

    def sync(self):
        self.context.sync()


_cpu = None


def cpu_backend():
    global _cpu
    if _cpu is None:
        _cpu = CpuBackend()
    return _cpu


# ----------------------------------------------------------------------------------------------------------------------
# trees
# ----------------------------------------------------------------------------------------------------------------------
_cache = {}


def _cloud(n, seed):
    """clustered cloud in the unit cube: Gaussian blobs of very different widths over a thin uniform background, and a
    few particles in every corner -- so the tree mixes deep and shallow leaves and is resolved up to the last key"""
    rng = np.random.default_rng(seed)
    nb = max(n // 10, 1)
    parts = [rng.uniform(0, 1, (nb, 3))]
    rest = n - nb
    centers = rng.uniform(0.1, 0.9, (6, 3))
    widths = [0.2, 0.05, 0.01, 0.002, 0.08, 0.0005]
    for c, w in zip(centers, widths):
        parts.append(rng.normal(c, w, (rest // 6 + 1, 3)))
    corners = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], float)
    parts.append(np.repeat(corners, 4, axis=0) + rng.uniform(-1e-4, 1e-4, (32, 3)))
    pts = np.clip(np.concatenate(parts), 0.0, np.nextafter(1.0, 0.0))
    return np.ascontiguousarray(pts.T)


def cloud_tree(oracle, kb, n, bucket, seed=1, curve=orc.HILBERT):
    """(sorted particle keys, leaves, leaf counts) of the converged cornerstone tree of a clustered cloud"""
    key = ("cloud", kb, n, bucket, seed, curve)
    if key not in _cache:
        pts = _cloud(n, seed)
        keys = np.sort(oracle.compute_sfc_keys(curve, kb, pts[0], pts[1], pts[2], orc.Box([0, 1])))
        leaves, counts = oracle.compute_octree(keys, bucket)
        _cache[key] = (keys, leaves, counts)
    return _cache[key]


def linked(oracle, leaves):
    key = ("linked", leaves.dtype.itemsize, leaves.tobytes())
    if key not in _cache:
        _cache[key] = oracle.build_octree(leaves)
    return _cache[key]


def split_tree(kb, num_splits, seed, deep=False):
    """a cornerstone leaf array made by splitting a leaf num_splits times (1 + 7 * num_splits leaves): for the leaf counts
    either side of a 256-thread workgroup (253, 260), which no particle cloud hits on purpose.  deep: always the last
    child of the last split, one branch down to the maximum depth."""
    rng = np.random.default_rng(seed)
    leaves = [0, orc.end_key(kb)]
    at = 0
    for _ in range(num_splits):
        if deep:
            i = at
        else:
            ok = [j for j in range(len(leaves) - 1) if leaves[j + 1] - leaves[j] >= 8]
            i = int(ok[int(rng.integers(0, len(ok)))])
        a, b = leaves[i], leaves[i + 1]
        if b - a < 8:
            break
        step = (b - a) // 8
        leaves[i + 1:i + 1] = [a + s * step for s in range(1, 8)]
        at = i + int(rng.integers(0, 8)) if deep else 0
    return np.array(leaves, dtype=orc.key_dtype(kb))


def leaf_levels(leaves):
    """tree level of every leaf: its key span is 8^(maxLevel - level)"""
    kb = leaves.dtype.itemsize * 8
    span = np.diff(leaves.astype(np.uint64))
    return orc.max_level(kb) - (bit_length(span) - 1) // 3


def bit_length(x):
    """number of significant bits of every element of an unsigned array (0 for 0), exact for all 64 bits"""
    x = np.asarray(x).astype(np.uint64)
    n = np.zeros(x.shape, np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        m = (x >> np.uint64(s)) != 0
        n[m] += s
        x = np.where(m, x >> np.uint64(s), x)
    return n + (x != 0)


def sample_keys(rng, leaves, n):
    """n query keys around a leaf array: leaf keys (first, last = the end key, and random ones, some several times), the
    keys one below and one above a leaf key, keys strictly inside leaves and arbitrary keys"""
    kdt = leaves.dtype
    if n == 0:
        return np.zeros(0, kdt)
    l64 = leaves.astype(np.uint64)
    pick = l64[rng.integers(0, leaves.size, n)]
    kind = rng.integers(0, 6, n)
    inner = rng.integers(0, leaves.size - 1, n)
    inside = l64[inner] + (rng.integers(0, 1 << 62, n).astype(np.uint64) % (l64[inner + 1] - l64[inner]))
    anywhere = rng.integers(0, int(l64[-1]), n, dtype=np.uint64)
    out = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4],
                    [pick, np.where(pick > 0, pick - np.uint64(1), pick), np.minimum(pick + np.uint64(1), l64[-1]),
                     inside, anywhere], pick)
    fixed = [l64[0], l64[-1], l64[-1] - np.uint64(1), l64[1], l64[1], l64[-2], l64[-2] + np.uint64(1)]
    for i, v in enumerate(fixed[:n]):
        out[(i * 37) % n if n > 7 else i] = v
    return out.astype(kdt)


# ----------------------------------------------------------------------------------------------------------------------
# models
# ----------------------------------------------------------------------------------------------------------------------
def keys_missing_model(leaves, keys):
    """cstone_hip.h, keys_missing: flags[i] = 1 if keys[i] is not one of leaves[0 .. num_leaves] -- checkTreelets
    (R/focus/exchange_focus.hpp:104-115): k != leaves[findNodeAbove(leaves, nNodes(leaves), k)], findNodeAbove = lower
    bound (R/tree/csarray.hpp:87-90) over the first num_leaves keys, so the index reaches num_leaves: the end key"""
    at = np.searchsorted(leaves[:-1], keys, side="left")
    return (leaves[at] != keys).astype(np.uint32)


def partition_keys_model(keys, flags):
    """cstone_hip.h, partition_keys: keys with flag 1 to set_out[scan[i]], the others to unset_out[i - scan[i]], scan =
    exclusive scan of the flags -- a stable partition (pruneTreelets, R/focus/exchange_focus.hpp:118-129, std::remove_if)"""
    return keys[flags != 0], keys[flags == 0]


def zero_ops_model(leaves, keys, node_ops):
    """cstone_hip.h, zero_ops_at_keys: node_ops[findNodeAbove(leaves, num_leaves + 1, keys[i])] = 0
    (exchangeRejectedKeys, R/focus/exchange_focus.hpp:186-190); keys <= leaves[num_leaves]"""
    out = node_ops.copy()
    out[np.searchsorted(leaves, keys, side="left")] = 0
    return out


def locate_nodes_model(keys, prefixes, level_range):
    """cstone_hip.h, locate_nodes = locateNode(startKey, endKey, ...) (R/tree/octree.hpp:216-241): prefixLength =
    countLeadingZeros(end - start - 1) - unusedBits; nodeKey = start's first prefixLength bits behind a placeholder bit
    (encodePlaceholderBit); level = prefixLength / 3; lower bound of nodeKey among the prefixes of that level; found if
    that position is not num_nodes and holds nodeKey.  end <= start: num_nodes (header)"""
    kb = keys.dtype.itemsize * 8
    ml = orc.max_level(kb)
    num_nodes = int(level_range[ml + 1])
    start, end = keys[:-1].astype(np.uint64), keys[1:].astype(np.uint64)
    out = np.full(start.size, num_nodes, np.int32)
    valid = end > start
    diff = np.where(valid, end - start - np.uint64(1), np.uint64(0))
    plen = (kb - bit_length(diff)) - (kb - 3 * ml)   # leading zeros in a kb-bit word, less the unused bits
    want = (np.uint64(1) << plen.astype(np.uint64)) | (start >> (3 * ml - plen).astype(np.uint64))
    level = plen // 3
    pre = prefixes.astype(np.uint64)
    for lv in np.unique(level[valid]):
        sel = np.nonzero(valid & (level == lv))[0]
        a, b = int(level_range[lv]), int(level_range[lv + 1])
        at = a + np.searchsorted(pre[a:b], want[sel], side="left")
        hit = at != num_nodes
        hit[hit] = pre[at[hit]] == want[sel][hit]
        out[sel[hit]] = at[hit]
    return out


def node_layout_model(counts, flags, first, last):
    """cstone_hip.h, node_layout = computeNodeLayout (R/domain/layout.hpp:150-165): exclusive scan, in LocalIndex = u32
    arithmetic, of counts[i] where the leaf is assigned (first <= i < last) or flagged as halo, 0 elsewhere"""
    i = np.arange(counts.size)
    present = ((i >= first) & (i < last)) | (flags != 0)
    c = np.where(present, counts, 0).astype(np.uint64)
    return (np.concatenate([np.zeros(1, np.uint64), np.cumsum(c, dtype=np.uint64)]) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def ranges_from_keys_model(leaves, layout, pairs):
    """cstone_hip.h, ranges_from_keys: the serving side of exchangeRequestKeys (R/domain/exchange_keys.hpp:98-108): range r
    = [layout[findNodeAbove(leaves, pairs[2r])], layout[findNodeAbove(leaves, pairs[2r+1])]), all num_leaves + 1 keys
    searched; offsets = the starts, scan = exclusive scan of the lengths with the total behind it"""
    lo = layout[np.searchsorted(leaves, pairs[0::2], side="left")]
    hi = layout[np.searchsorted(leaves, pairs[1::2], side="left")]
    length = (hi.astype(np.int64) - lo.astype(np.int64)).astype(np.uint64)
    scan = (np.concatenate([np.zeros(1, np.uint64), np.cumsum(length, dtype=np.uint64)]) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return lo.astype(np.uint32), scan


def range_indices(offsets, scan):
    """source index of every buffer element of gatherRanges (R/halos/gather_halos_gpu.cu:26-40):
    offsets[r] + i - scan[r] for scan[r] <= i < scan[r + 1]"""
    lengths = np.diff(scan.astype(np.int64))
    r = np.repeat(np.arange(lengths.size), lengths)
    return offsets.astype(np.int64)[r] + np.arange(int(scan[-1])) - scan.astype(np.int64)[r]


def gather_rows_model(offsets, scan, arrays):
    """cstone_hip.h, gather_ranges_rows: rows[i * num_arrays + a] = src[a][range_offsets[r] + i - range_scan[r]]"""
    idx = range_indices(offsets, scan)
    return np.stack([a[idx] for a in arrays], axis=1).reshape(-1)


def scatter_rows_model(rows, num_arrays, dst, dst_offset):
    """cstone_hip.h, scatter_rows: dst[a][dst_offset + i] = rows[i * num_arrays + a], nothing else written"""
    out = [d.copy() for d in dst]
    r = rows.reshape(-1, num_arrays)
    for a in range(num_arrays):
        out[a][dst_offset:dst_offset + r.shape[0]] = r[:, a]
    return out


def gather_tables_model(map_, a, n_a, b, n_b, c, n_c):
    """cstone_hip.h, gather_tables_u32: out = a[map[:n_a]] (zeros when a is null) | b[map[n_a : n_a + n_b]] | c[:n_c]"""
    first = a[map_[:n_a]] if a is not None else np.zeros(n_a, np.uint32)
    return np.concatenate([first, b[map_[n_a:n_a + n_b]] if n_b else np.zeros(0, np.uint32),
                           c[:n_c] if n_c else np.zeros(0, np.uint32)]).astype(np.uint32)


def focus_update_model(oracle, octree, counts, macs, focus_start, focus_end, bucket, forced):
    """cstone_hip.h, focus_update_ops = the decision part of CombinedUpdate::updateFocus (R/focus/octree_focus.hpp:97-122):
    rebalanceDecisionEssential, enforceKeys, protectAncestors (the oracle's restatements, checked against the reference's
    functions in test_focus.py), the leaves' ops in leaf order scanned exclusively; converged: protectAncestors' verdict
    (every op is 1), but with status 1 (cancelMerge) "every leaf keeps", and 0 with status >= 2 (:109-121).
    NOT independent evidence on the cpu leg: the CPU restatement behind the ABI calls the same three oracle functions, so
    there only these few lines of glue (order of the steps, leaf order, scan, the rules for converged) are compared; the
    three functions themselves are checked against the reference's in test_focus.py.  The hip leg compares the kernels."""
    ops = oracle.essential_ops(octree, counts, macs, focus_start, focus_end, bucket)
    status = 0
    if forced.size:
        ops, status = oracle.enforce_keys(forced, octree, ops)
    ops, conv = oracle.protect_ancestors(octree, ops)
    leaf = ops[octree["leaf_to_internal"][octree["num_internal"]:]]
    keep = int((leaf == 1).all())
    converged = int(conv)
    if status == 1:
        converged = keep
    if status >= 2:
        converged = 0
    scan = np.concatenate([[0], np.cumsum(leaf.astype(np.int64))]).astype(np.int32)
    return ops, scan, [status, converged, keep, int(scan[-1])]


def leaf_boxes(oracle, curve, leaves, box):
    """centre and half size (float64) of every leaf: centerAndSize (R/sfc/box.hpp:334-351) of its integer box"""
    kb = leaves.dtype.itemsize * 8
    lv = leaf_levels(leaves)
    ib = np.array([oracle.node_ibox(curve, kb, int(k), int(l)) for k, l in zip(leaves[:-1], lv)], np.float64)
    lengths = box.lim[1::2] - box.lim[0::2]
    half = 0.5 * (1.0 / (1 << orc.max_level(kb))) * lengths
    center = box.lim[0::2] + (ib[:, 1::2] + ib[:, 0::2]) * half
    size = (ib[:, 1::2] - ib[:, 0::2]) * half
    return center, size


def peers_model(leaves, center, size, box, assignment, my_rank, inv_theta_eff, margins=(1e-9, 1e-6)):
    """cstone_hip.h, find_peers_mac, as the all-pairs check of the reference's unit test (findPeersAll2All,
    test/unit/traversal/peers.cpp:43-73): rank r != my_rank is a peer iff a leaf of its range and a leaf of mine fail
    minVecMacMutual (R/traversal/macs.hpp:171-194; minDistance with applyPbc, R/traversal/boxoverlap.hpp:208-217,
    R/sfc/box.hpp:195-206), in float64.  Also returns, for each of the relative `margins`, the number of leaf pairs
    that close to a MAC threshold: their verdict would depend on the order of the operations (in double for the first
    margin, in float for the second)."""
    num_ranks = assignment.size - 1
    lengths = box.lim[1::2] - box.lim[0::2]
    inv = 1.0 / lengths
    pbc = (box.bc == 1).astype(np.float64)
    inv_theta = float(np.float32(inv_theta_eff))
    first = int(np.searchsorted(leaves, assignment[my_rank]))
    last = int(np.searchsorted(leaves, assignment[my_rank + 1]))
    rank_of = np.searchsorted(assignment, leaves[:-1], side="right") - 1
    foreign = np.ones(leaves.size - 1, bool)
    foreign[first:last] = False
    j = np.nonzero(foreign)[0]
    peers = np.zeros(num_ranks, np.int32)
    near = [0] * len(margins)
    mac_j = (size[j].max(axis=1) * 2 * inv_theta) ** 2

    def dist2(x, bc, bs):  # squared distance of the points x to the boxes (bc, bs)
        d = bc - x
        d = np.abs(d - pbc * lengths * np.rint(d * inv)) - bs
        d = (d + np.abs(d)) * 0.5
        return d[..., 0] ** 2 + (d[..., 1] ** 2 + d[..., 2] ** 2)

    for i0 in range(first, last, 512):
        i = np.arange(i0, min(i0 + 512, last))
        ci, si = center[i][:, None, :], size[i][:, None, :]
        cj, sj = center[j][None, :, :], size[j][None, :, :]
        mac_i = ((size[i].max(axis=1) * 2 * inv_theta) ** 2)[:, None]
        d_a = dist2(cj, ci, si)  # A (mine) = target, B = source
        d_b = dist2(ci, cj, sj)
        fail = ~((d_a > mac_j[None, :]) & (d_b > mac_i))
        for m, margin in enumerate(margins):
            near[m] += int(np.count_nonzero(np.abs(d_a - mac_j[None, :]) <= margin * mac_j[None, :]))
            near[m] += int(np.count_nonzero(np.abs(d_b - mac_i) <= margin * mac_i))
        peers[np.unique(rank_of[j[fail.any(axis=0)]])] = 1
    return peers, near
