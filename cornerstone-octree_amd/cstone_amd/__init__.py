"""Python plumbing for libcstone_hip.so (ctypes over the C ABI of include/cstone_hip.h).

This is NOT the product: the product is the shared library and the C++20 headers in
cornerstone-octree_amd/include/.  The module exists so that tests/, bench.py and smoke() can drive
the C ABI with torch tensors as device buffers (torch = device memory + streams + torch.distributed).
There is NO fallback: if the library is missing or a call fails, an exception is raised.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
LIBPATH = os.path.join(PKG, "lib", "libcstone_hip.so")

MORTON, HILBERT = 0, 1

STAGES = {
    "encode": 0, "sort_hist": 1, "sort_pass": 2, "gather": 3, "node_counts": 4, "rebalance": 5, "link_octree": 6,
    "halos": 7, "neighbors": 8, "minmax": 9, "sort_pass_iota": 10, "resort_bins": 11, "resort_leaves": 12, "gather_h": 13, "place": 14,
    "multipoles": 15, "gravity": 16, "adapt_h": 17, "fof": 18,
}

EXPORTS = [
    "cstone_hip_ctx_create", "cstone_hip_ctx_destroy", "cstone_hip_ctx_sync", "cstone_hip_last_error",
    "cstone_hip_device_info", "cstone_hip_malloc", "cstone_hip_free", "cstone_hip_memcpy_h2d",
    "cstone_hip_memcpy_d2h", "cstone_hip_memcpy_d2d", "cstone_hip_memset", "cstone_hip_profile_enable", "cstone_hip_profile_markers", "cstone_hip_domain_mr_sync_grav", "cstone_hip_domain_mr_update_expansion_centers", "cstone_hip_add_macs", "cstone_hip_halo_request_rows", "cstone_hip_peer_range_counts", "cstone_hip_adjacent_difference_u32", "cstone_hip_offsets_from_counts_u32", "cstone_hip_domain_sync_grav", "cstone_hip_domain_update_expansion_centers", "cstone_hip_gather_tables_u32",
    "cstone_hip_profile_reset", "cstone_hip_profile_get", "cstone_hip_profile_get_spread", "cstone_hip_compute_sfc_keys",
    "cstone_hip_sort_pairs_temp_bytes", "cstone_hip_sort_pairs", "cstone_hip_sort_keys_ordering", "cstone_hip_sfc_keys_and_ordering", "cstone_hip_sfc_keys_and_ordering_partial", "cstone_hip_sequence_u32", "cstone_hip_gather",
    "cstone_hip_scatter", "cstone_hip_gather_scatter", "cstone_hip_merge_positions", "cstone_hip_minmax", "cstone_hip_minmax_arrays", "cstone_hip_exclusive_scan_u32", "cstone_hip_inclusive_scan_u32", "cstone_hip_lower_bound",
    "cstone_hip_compute_node_counts", "cstone_hip_compute_node_counts_guided", "cstone_hip_compute_node_ops", "cstone_hip_rebalance_tree",
    "cstone_hip_update_octree", "cstone_hip_compute_octree", "cstone_hip_build_octree", "cstone_hip_upsweep_sum",
    "cstone_hip_node_centers", "cstone_hip_halo_radii", "cstone_hip_find_halos", "cstone_hip_find_neighbors",
    "cstone_hip_halo_boxes", "cstone_hip_halo_boxes_foreign", "cstone_hip_find_overlaps", "cstone_hip_compute_fixed_groups",
    "cstone_hip_compute_group_splits", "cstone_hip_find_neighbors_groups",
    "cstone_hip_domain_create", "cstone_hip_domain_destroy", "cstone_hip_domain_sync", "cstone_hip_domain_view_get",
    "cstone_hip_domain_set_halo_factor", "cstone_hip_domain_mr_create", "cstone_hip_domain_mr_destroy",
    "cstone_hip_domain_mr_sync", "cstone_hip_domain_mr_sync_props", "cstone_hip_domain_mr_sync_keys", "cstone_hip_domain_mr_view_get", "cstone_hip_domain_mr_set_halo_factor", "cstone_hip_domain_mr_exchange_halos", "cstone_hip_domain_mr_reapply_sync",
    "cstone_hip_domain_reapply_sync", "cstone_hip_domain_stats_get",
    "cstone_hip_domain_mr_octree_get",
    "cstone_hip_fill", "cstone_hip_scale", "cstone_hip_increment", "cstone_hip_count_equal", "cstone_hip_reduce_sum",
    "cstone_hip_max_norm_square", "cstone_hip_segment_max", "cstone_hip_gather_ranges", "cstone_hip_lower_bound_value",
    "cstone_hip_sort_keys", "cstone_hip_rebalance_decision_essential", "cstone_hip_mac_refine_decision",
    "cstone_hip_protect_ancestors", "cstone_hip_enforce_keys", "cstone_hip_range_count", "cstone_hip_mark_macs",
    "cstone_hip_count_sfc_gaps", "cstone_hip_fill_sfc_gaps", "cstone_hip_geo_mac_spheres", "cstone_hip_set_mac",
    "cstone_hip_move_centers", "cstone_hip_leaf_source_centers", "cstone_hip_upsweep_centers",
    "cstone_hip_comm_rccl_unique_id", "cstone_hip_comm_rccl_create", "cstone_hip_comm_rccl_ops",
    "cstone_hip_comm_rccl_destroy", "cstone_hip_create_binary_tree",
    # the device work behind the locally essential tree's host state machine (csrc/let.hpp)
    "cstone_hip_raise", "cstone_hip_find_peers_mac", "cstone_hip_keys_missing", "cstone_hip_partition_keys",
    "cstone_hip_zero_ops_at_keys", "cstone_hip_locate_nodes", "cstone_hip_node_layout", "cstone_hip_halo_requests",
    "cstone_hip_ranges_from_keys", "cstone_hip_domain_mr_set_halo_mode", "cstone_hip_domain_mr_set_theta",
    "cstone_hip_upload", "cstone_hip_focus_update_ops", "cstone_hip_find_neighbors_stats",
    "cstone_hip_gather_multi", "cstone_hip_domain_sync_scratch", "cstone_hip_gather_ranges_rows",
    "cstone_hip_scatter_rows", "cstone_hip_build_octree_bounded", "cstone_hip_upsweep_sum_bounded",
    "cstone_hip_lower_bound_u32", "cstone_hip_sequence_u64", "cstone_hip_scan_u32_to_u64",
    "cstone_hip_domain_set_sort_mode", "cstone_hip_domain_set_speculative_box", "cstone_hip_test_hooks",
    "cstone_hip_domain_mr_set_sort_mode", "cstone_hip_find_neighbors_interleaved",
    # Barnes-Hut gravity (csrc/gravity.hip)
    "cstone_hip_upsweep_multipoles", "cstone_hip_compute_gravity", "cstone_hip_domain_compute_gravity",
    # ... on a locally essential tree and on several ranks (csrc/let.hpp, FocusLet::updateMultipoles)
    "cstone_hip_upsweep_multipoles_nodes", "cstone_hip_compute_gravity_let", "cstone_hip_domain_mr_compute_gravity",
    "cstone_hip_domain_mr_multipoles_get",
    # ... with per-particle softening lengths, and the all-pairs direct sum
    "cstone_hip_compute_gravity_h", "cstone_hip_compute_gravity_let_h", "cstone_hip_direct_gravity",
    "cstone_hip_domain_compute_gravity_h", "cstone_hip_domain_mr_compute_gravity_h",
    # ... at order 3: the octupoles beside the multipoles
    "cstone_hip_upsweep_octupoles", "cstone_hip_upsweep_octupoles_nodes", "cstone_hip_compute_gravity_o3",
    "cstone_hip_domain_mr_octupoles_get",
    # adaptive smoothing lengths: h iterated to a neighbour count inside one kernel (csrc/adapt_h.hip)
    "cstone_hip_adapt_smoothing_lengths", "cstone_hip_domain_adapt_h", "cstone_hip_domain_mr_adapt_h",
    # friends-of-friends groups: lock-free union-find on the neighbour walk (csrc/fof.hip)
    "cstone_hip_friends_of_friends", "cstone_hip_fof_catalog", "cstone_hip_domain_fof",
    # ... across ranks: the lowering step of a round and the collective call (csrc/fof.hip, csrc/domain_mr.hip)
    "cstone_hip_fof_lower_labels", "cstone_hip_domain_mr_fof",
    # the group catalogue: mass, centre, velocity, radius of every group (csrc/fof_props.hip, csrc/domain_mr.hip)
    "cstone_hip_fof_group_properties", "cstone_hip_domain_fof_properties", "cstone_hip_domain_mr_fof_catalog",
    # sphere queries at arbitrary points: radial profiles and spherical-overdensity masses (csrc/sphere.hip)
    "cstone_hip_sphere_profiles", "cstone_hip_spherical_overdensity", "cstone_hip_domain_sphere_profiles",
    "cstone_hip_domain_mr_sphere_profiles",
    # exact k nearest neighbours at arbitrary points (csrc/knn.hip)
    "cstone_hip_knn", "cstone_hip_domain_knn", "cstone_hip_domain_mr_knn", "cstone_hip_knn_mr_chunk_queries",
    "cstone_hip_domain_mr_knn_last",
    # pair counts in radial bins and the two-point correlation function (csrc/pair_counts.hip)
    "cstone_hip_pair_counts", "cstone_hip_pair_counts_cross", "cstone_hip_domain_pair_counts",
    "cstone_hip_domain_pair_counts_cross", "cstone_hip_domain_mr_pair_counts", "cstone_hip_domain_mr_pair_counts_cross",
    "cstone_hip_xi_natural",
]

PAIR_MAX_BINS = 64  # CSTONE_PAIR_MAX_BINS

FOF_GROUP_WIDE, FOF_GROUP_MASSLESS = 0x1, 0x2  # CSTONE_FOF_GROUP_*: the flags of the group catalogue

SPHERE_MAX_BINS = 64  # CSTONE_SPHERE_MAX_BINS
# CSTONE_SPHERE_TOO_WIDE (profiles and overdensity), CSTONE_SO_NOT_REACHED, CSTONE_SO_UNRESOLVED (overdensity)
SPHERE_TOO_WIDE, SO_NOT_REACHED, SO_UNRESOLVED = 0x1, 0x2, 0x4

KNN_MAX_K = 256  # CSTONE_KNN_MAX_K
KNN_MR_GATHER_BYTES = 256 << 20  # CSTONE_KNN_MR_GATHER_BYTES: the cap on the receive buffer of one all_gather of rows
KNN_NONE = 0xFFFFFFFF  # what an unfilled slot of neighbors holds, and the query_self that excludes nothing

FOF_MR_DEFAULT_ROUNDS = 4096  # CSTONE_FOF_MR_DEFAULT_ROUNDS: what max_rounds = 0 means to cstone_hip_domain_mr_fof

# status word of the adapt calls: number of walks in bits 0-7, then the CSTONE_ADAPT_H_* flags
ADAPT_H_WALKS_MASK, ADAPT_H_NOT_CONVERGED, ADAPT_H_CAPPED, ADAPT_H_STALLED = 0xFF, 0x100, 0x200, 0x400

GRAVITY_GROUP_TOL = 2.0  # CSTONE_GRAVITY_GROUP_TOL: tol_factor of the target groups of cstone_hip_domain_compute_gravity


class CBox(C.Structure):
    _fields_ = [("lim", C.c_double * 6), ("bc", C.c_int32 * 3), ("pad_", C.c_int32)]


def make_cbox(lim, bc=(0, 0, 0)):
    b = CBox()
    for i in range(6):
        b.lim[i] = float(lim[i])
    for i in range(3):
        b.bc[i] = int(bc[i])
    return b


PARTIAL_SORT_RUN_LIMIT = 192  # CSTONE_PARTIAL_SORT_RUN_LIMIT


class PartialSortResult(C.Structure):
    _fields_ = [("run_too_long", C.c_int32), ("finished", C.c_int32), ("extents_measured", C.c_int32),
                ("pad_", C.c_int32), ("extents", C.c_double * 6)]


class CstoneError(RuntimeError):
    pass


def max_level(key_bits):
    return {32: 10, 64: 21}[key_bits]


def load_library():
    """dlopen the product library; raises if it has not been built (no fallback of any kind)"""
    path = os.environ.get("CSTONE_HIP_LIB", LIBPATH)  # tuning builds; the default is the in-tree product library
    if not os.path.exists(path):
        raise CstoneError(f"{LIBPATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          f"or `make -C cornerstone-octree_amd`")
    # torch first: it brings its own libamdhip64, and a process must hold ONE HIP runtime -- with the library's
    # /opt/rocm copy loaded before torch's, the second runtime finds no device ("no ROCm-capable device is detected")
    import torch  # noqa: F401

    lib = C.CDLL(path)
    lib.cstone_hip_last_error.restype = C.c_char_p
    lib.cstone_hip_sort_pairs_temp_bytes.restype = C.c_size_t
    # friends-of-friends across ranks: (ctx, component, n, first, last, labels, changed) and (domain, x, y, z,
    # linking_length, max_rounds, labels, group_sizes, num_groups*, rounds*)
    lib.cstone_hip_fof_lower_labels.restype = C.c_int
    lib.cstone_hip_fof_lower_labels.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                                C.c_void_p]
    lib.cstone_hip_domain_mr_fof.restype = C.c_int
    lib.cstone_hip_domain_mr_fof.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_uint32,
                                             C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    # the group catalogue: (ctx, real_bits, mass_bits, x, y, z, m, vx, vy, vz, box*, group_offsets, members, num_groups,
    # mass, center, velocity, radius, flags); the domain's call has the domain and mass_bits behind m instead
    lib.cstone_hip_fof_group_properties.restype = C.c_int
    lib.cstone_hip_fof_group_properties.argtypes = ([C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 10 + [C.c_uint32] +
                                                    [C.c_void_p] * 5)
    lib.cstone_hip_domain_fof_properties.restype = C.c_int
    lib.cstone_hip_domain_fof_properties.argtypes = ([C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 5 + [C.c_uint32] +
                                                     [C.c_void_p] * 5)
    # (domain, x, y, z, m, mass_bits, vx, vy, vz, labels, min_members, capacity, group_labels, group_sizes, mass, center,
    # velocity, radius, flags, num_groups*)
    lib.cstone_hip_domain_mr_fof_catalog.restype = C.c_int
    lib.cstone_hip_domain_mr_fof_catalog.argtypes = ([C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 4 +
                                                     [C.c_uint64, C.c_size_t] + [C.c_void_p] * 7 + [C.POINTER(C.c_uint32)])
    # sphere queries: (ctx, real_bits, mass_bits, x, y, z, w, first, last, box*, child_offsets, internal_to_leaf, layout,
    # centers, sizes, query_centers, query_scale, num_queries, edges*, num_bins, counts, sums, flags); the finish: (ctx,
    # real_bits, query_scale, num_queries, edges*, num_bins, sums, profile_flags, rho, r_delta, m_delta, flags); the
    # domains': (domain, x, y, z, w, mass_bits, query_centers, query_scale, num_queries, edges*, num_bins, counts, sums, flags)
    lib.cstone_hip_sphere_profiles.restype = C.c_int
    lib.cstone_hip_sphere_profiles.argtypes = ([C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_uint32] * 2 +
                                               [C.c_void_p] * 8 + [C.c_uint32, C.POINTER(C.c_double), C.c_int] +
                                               [C.c_void_p] * 3)
    lib.cstone_hip_spherical_overdensity.restype = C.c_int
    lib.cstone_hip_spherical_overdensity.argtypes = ([C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.POINTER(C.c_double),
                                                      C.c_int, C.c_void_p, C.c_void_p, C.c_double] + [C.c_void_p] * 3)
    for fn in (lib.cstone_hip_domain_sphere_profiles, lib.cstone_hip_domain_mr_sphere_profiles):
        fn.restype = C.c_int
        fn.argtypes = ([C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 2 + [C.c_uint32, C.POINTER(C.c_double), C.c_int] +
                       [C.c_void_p] * 3)
    # k nearest neighbours: (ctx, real_bits, x, y, z, first, last, box*, child_offsets, internal_to_leaf, layout, centers,
    # sizes, query_centers, query_rmax, query_self, num_queries, k, neighbors, dist2, counts); the domain's: (domain, x, y,
    # z, query_centers, query_rmax, query_self, num_queries, k, neighbors, dist2, counts)
    lib.cstone_hip_knn.restype = C.c_int
    lib.cstone_hip_knn.argtypes = ([C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_uint32] * 2 + [C.c_void_p] * 9 +
                                   [C.c_uint32] * 2 + [C.c_void_p] * 3)
    lib.cstone_hip_domain_knn.restype = C.c_int
    lib.cstone_hip_domain_knn.argtypes = [C.c_void_p] * 7 + [C.c_uint32] * 2 + [C.c_void_p] * 3
    # across ranks: (domain, x, y, z, query_centers, query_rmax, num_queries, k, ids, dist2, counts); the chunk rule
    # (num_queries, k, num_ranks, cap_bytes) -> queries per all_gather; (domain, num_chunks*, gather_bytes*) of the last call
    lib.cstone_hip_domain_mr_knn.restype = C.c_int
    lib.cstone_hip_domain_mr_knn.argtypes = [C.c_void_p] * 6 + [C.c_uint32] * 2 + [C.c_void_p] * 3
    lib.cstone_hip_knn_mr_chunk_queries.restype = C.c_uint32
    lib.cstone_hip_knn_mr_chunk_queries.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_uint64]
    lib.cstone_hip_domain_mr_knn_last.restype = C.c_int
    lib.cstone_hip_domain_mr_knn_last.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    # pair counts: (ctx, real_bits, w_bits, x, y, z, w, first, last, t_first, t_last, box*, child_offsets,
    # internal_to_leaf, layout, centers, sizes, edges*, num_bins, counts, sums, stats*); cross: (ctx, real_bits, w_bits, x,
    # y, z, w, first, last, box*, child_offsets, internal_to_leaf, layout, centers, sizes, query_centers, query_w,
    # num_queries, edges*, num_bins, counts, sums, stats*); the domains': (domain, x, y, z, w, w_bits, [query_centers,
    # query_w, num_queries,] edges*, num_bins, counts, sums, stats*); xi: (counts*, edges*, num_bins, n_targets,
    # n_partners, volume, xi*), all host
    stats = C.POINTER(C.c_uint64)
    lib.cstone_hip_pair_counts.restype = C.c_int
    lib.cstone_hip_pair_counts.argtypes = ([C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_uint32] * 4 +
                                           [C.c_void_p] * 6 + [C.POINTER(C.c_double), C.c_int] + [C.c_void_p] * 2 + [stats])
    lib.cstone_hip_pair_counts_cross.restype = C.c_int
    lib.cstone_hip_pair_counts_cross.argtypes = ([C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_uint32] * 2 +
                                                 [C.c_void_p] * 8 + [C.c_uint32, C.POINTER(C.c_double), C.c_int] +
                                                 [C.c_void_p] * 2 + [stats])
    for fn in (lib.cstone_hip_domain_pair_counts, lib.cstone_hip_domain_mr_pair_counts):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p] * 5 + [C.c_int, C.POINTER(C.c_double), C.c_int] + [C.c_void_p] * 2 + [stats]
    for fn in (lib.cstone_hip_domain_pair_counts_cross, lib.cstone_hip_domain_mr_pair_counts_cross):
        fn.restype = C.c_int
        fn.argtypes = ([C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 2 + [C.c_uint32, C.POINTER(C.c_double), C.c_int] +
                       [C.c_void_p] * 2 + [stats])
    lib.cstone_hip_xi_natural.restype = C.c_int
    lib.cstone_hip_xi_natural.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.c_int, C.c_double, C.c_double,
                                          C.c_double, C.POINTER(C.c_double)]
    return lib


def xi_natural(counts, edges, n_targets, n_partners, volume):
    """cstone_hip_xi_natural (host, float64): the natural estimator of the two-point correlation function in a PERIODIC
    box of the given volume from pair counts [NB] over the bin edges [NB + 1]:
    xi[b] = counts[b] / (n_targets * n_partners * (4 pi / 3) (edges[b+1]^3 - edges[b]^3) / volume) - 1; for auto counts
    pass n_partners = n - 1.  A bin of zero shell volume or zero expected pairs gives NaN.  Returns a float64 array"""
    lib = load_library()
    e, nb = sphere_edges(edges)
    c = [int(v) for v in (counts.tolist() if hasattr(counts, "tolist") else counts)]
    if len(c) != nb:
        raise CstoneError(f"xi_natural: {len(c)} counts for {nb} bins")
    carr = (C.c_uint64 * max(nb, 1))(*c)
    out = (C.c_double * max(nb, 1))()
    rc = lib.cstone_hip_xi_natural(carr, e, nb, float(n_targets), float(n_partners), float(volume), out)
    if rc != 0:
        raise CstoneError(f"xi_natural failed ({rc}): 1 .. {PAIR_MAX_BINS} bins with finite, non-negative, strictly "
                          f"ascending edges are taken")
    return np.array(out[:nb], dtype=np.float64)


def sphere_edges(edges):
    """(host array of C doubles, number of bins) of a sequence of bin edges, as the sphere calls take them"""
    e = [float(v) for v in edges]
    return (C.c_double * max(len(e), 1))(*e), len(e) - 1


def _opt(t):
    """data pointer of a tensor, or None"""
    return None if t is None else t.data_ptr()


def _torch():
    import torch

    return torch


def _ptr(t):
    if t is None:
        return C.c_void_p(0)
    return C.c_void_p(t.data_ptr())


def key_torch_dtype(key_bits):
    torch = _torch()
    # torch has no unsigned 32/64 arithmetic types we need; keys live in int32/int64 storage (bit patterns)
    return {32: torch.int32, 64: torch.int64}[key_bits]


def keys_to_numpy(t, key_bits):
    a = t.cpu().numpy()
    return a.view(np.uint32 if key_bits == 32 else np.uint64)


def keys_from_numpy(a, device):
    torch = _torch()
    a = np.ascontiguousarray(a)
    signed = a.view(np.int32 if a.dtype.itemsize == 4 else np.int64)
    return torch.from_numpy(signed.copy()).to(device)


class Context:
    """One cstone_hip context bound to a torch device and (by default) torch's current stream."""

    def __init__(self, device=0, use_torch_stream=True):
        torch = _torch()
        self.lib = load_library()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if not torch.cuda.is_available():
            raise CstoneError("no GPU visible: libcstone_hip needs an MI355X (there is no CPU path)")
        torch.cuda.set_device(self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream if use_torch_stream else 0
        # the stream the library's work is ordered on, as torch sees it (None: a private stream of the library)
        self.stream_handle = stream if use_torch_stream else None
        self.h = C.c_void_p()
        rc = self.lib.cstone_hip_ctx_create(C.byref(self.h), C.c_int(self.device.index), C.c_void_p(stream),
                                            C.c_int(0 if use_torch_stream else 1))
        if rc != 0:
            self.lib.cstone_hip_last_error.restype = C.c_char_p
            why = self.lib.cstone_hip_last_error(C.c_void_p(None))
            raise CstoneError(f"cstone_hip_ctx_create failed: {rc} ({why.decode() if why else '?'})")

    def close(self):
        if getattr(self, "h", None):
            self.lib.cstone_hip_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        # not during interpreter shutdown: the HIP runtime may be gone by then (objects kept alive by a traceback are
        # collected that late), and the process is about to release everything anyway
        if sys is None or sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            msg = self.lib.cstone_hip_last_error(self.h)
            raise CstoneError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def sync(self):
        self._chk(self.lib.cstone_hip_ctx_sync(self.h), "ctx_sync")

    # ---- profiling
    def profile_enable(self, on=True):
        """True / 1: every stage; 2: only the stages of the kernels that move the particle arrays; False: off"""
        self._chk(self.lib.cstone_hip_profile_enable(self.h, C.c_int(int(on))), "profile_enable")

    def profile_markers(self, on=True):
        """roctx ranges "cstone:<stage>" around every stage (rocprofv3 --marker-trace)"""
        self._chk(self.lib.cstone_hip_profile_markers(self.h, C.c_int(int(on))), "profile_markers")

    def profile_reset(self):
        self._chk(self.lib.cstone_hip_profile_reset(self.h), "profile_reset")

    def profile_get(self, stage):
        ms, cnt = C.c_double(0), C.c_int(0)
        self._chk(self.lib.cstone_hip_profile_get(self.h, C.c_int(STAGES[stage]), C.byref(ms), C.byref(cnt)),
                  "profile_get")
        return ms.value, cnt.value

    def profile_spread(self, stage):
        """(min, median, max) ms of the individual brackets of a stage since the last reset"""
        lo, med, hi = C.c_double(0), C.c_double(0), C.c_double(0)
        self._chk(self.lib.cstone_hip_profile_get_spread(self.h, C.c_int(STAGES[stage]), C.byref(lo), C.byref(med),
                                                         C.byref(hi)), "profile_get_spread")
        return lo.value, med.value, hi.value

    # ---- keys
    def compute_sfc_keys(self, curve, key_bits, x, y, z, box, keys=None):
        torch = _torch()
        n = x.numel()
        if keys is None:
            keys = torch.zeros(n, dtype=key_torch_dtype(key_bits), device=x.device)
        rb = x.element_size() * 8
        self._chk(self.lib.cstone_hip_compute_sfc_keys(self.h, C.c_int(curve), C.c_int(key_bits), C.c_int(rb),
                                                       _ptr(x), _ptr(y), _ptr(z), _ptr(keys), C.c_size_t(n),
                                                       C.byref(box)), "compute_sfc_keys")
        return keys

    # ---- sort
    def sort_temp_bytes(self, key_bits, n):
        return int(self.lib.cstone_hip_sort_pairs_temp_bytes(C.c_int(key_bits), C.c_size_t(n)))

    def sort_pairs(self, keys, vals, keys_alt=None, vals_alt=None, temp=None):
        """in place; vals int32 storage holding uint32"""
        kb = keys.element_size() * 8
        n = keys.numel()
        tb = temp.numel() * temp.element_size() if temp is not None else 0
        self._chk(self.lib.cstone_hip_sort_pairs(self.h, C.c_int(kb), _ptr(keys), _ptr(vals), C.c_size_t(n),
                                                 _ptr(keys_alt), _ptr(vals_alt), _ptr(temp), C.c_size_t(tb)),
                  "sort_pairs")

    def sort_keys_ordering(self, keys):
        """sorts keys in place, returns the sorting permutation (int32 storage)"""
        torch = _torch()
        kb, n = keys.element_size() * 8, keys.numel()
        order = torch.empty(n, dtype=torch.int32, device=keys.device)
        ka, va = torch.empty_like(keys), torch.empty_like(order)
        tmp = torch.empty(max(1, self.sort_temp_bytes(kb, n)), dtype=torch.uint8, device=keys.device)
        self._chk(self.lib.cstone_hip_sort_keys_ordering(self.h, C.c_int(kb), _ptr(keys), _ptr(order), C.c_size_t(n),
                                                         _ptr(ka), _ptr(va), _ptr(tmp),
                                                         C.c_size_t(tmp.numel())), "sort_keys_ordering")
        return order

    def sfc_keys_and_ordering(self, curve, key_bits, x, y, z, box, keys=None):
        """(sorted keys, ordering): compute_sfc_keys + sort_keys_ordering in one call"""
        torch = _torch()
        n = x.numel()
        if keys is None:
            keys = torch.zeros(n, dtype=key_torch_dtype(key_bits), device=x.device)
        order = torch.empty(n, dtype=torch.int32, device=x.device)
        ka, va = torch.empty_like(keys), torch.empty_like(order)
        tmp = torch.empty(max(1, self.sort_temp_bytes(key_bits, n)), dtype=torch.uint8, device=x.device)
        self._chk(self.lib.cstone_hip_sfc_keys_and_ordering(self.h, C.c_int(curve), C.c_int(key_bits),
                                                            C.c_int(x.element_size() * 8), _ptr(x), _ptr(y), _ptr(z),
                                                            _ptr(keys), _ptr(order), C.c_size_t(n), C.byref(box),
                                                            _ptr(ka), _ptr(va), _ptr(tmp), C.c_size_t(tmp.numel())),
                  "sfc_keys_and_ordering")
        return keys, order

    def sfc_keys_and_ordering_partial(self, curve, key_bits, x, y, z, box, start_pass, keys=None, honour_markers=True,
                                      finish=True, temp=None):
        """(keys, ordering, info): sfc_keys_and_ordering with the radix passes from digit start_pass upward and the
        fix-up of the runs of equal high digits; info = dict(run_too_long, finished, extents (6 floats) or None)"""
        torch = _torch()
        n = x.numel()
        if keys is None:
            keys = torch.zeros(n, dtype=key_torch_dtype(key_bits), device=x.device)
        order = torch.empty(n, dtype=torch.int32, device=x.device)
        ka, va = torch.empty_like(keys), torch.empty_like(order)
        if temp is None:
            temp = torch.empty(max(1, self.sort_temp_bytes(key_bits, n)), dtype=torch.uint8, device=x.device)
        res = PartialSortResult()
        self._chk(self.lib.cstone_hip_sfc_keys_and_ordering_partial(
            self.h, C.c_int(curve), C.c_int(key_bits), C.c_int(x.element_size() * 8), _ptr(x), _ptr(y), _ptr(z),
            _ptr(keys), _ptr(order), C.c_size_t(n), C.byref(box), _ptr(ka), _ptr(va), _ptr(temp),
            C.c_size_t(temp.numel()), C.c_int(start_pass), C.c_int(int(bool(honour_markers))),
            C.c_int(int(bool(finish))), C.byref(res)), "sfc_keys_and_ordering_partial")
        info = {"run_too_long": bool(res.run_too_long), "finished": bool(res.finished),
                "extents": tuple(res.extents) if res.extents_measured else None}
        return keys, order, info

    def sequence(self, out, init=0):
        self._chk(self.lib.cstone_hip_sequence_u32(self.h, _ptr(out), C.c_size_t(out.numel()), C.c_uint32(init)),
                  "sequence_u32")

    def gather(self, map_, src, dst, elem_bytes=None, n=None):
        eb = elem_bytes or src.element_size()
        n = map_.numel() if n is None else n
        self._chk(self.lib.cstone_hip_gather(self.h, C.c_int(eb), _ptr(map_), C.c_size_t(n), _ptr(src), _ptr(dst)),
                  "gather")

    def scatter(self, map_, src, dst, elem_bytes=None):
        eb = elem_bytes or src.element_size()
        self._chk(self.lib.cstone_hip_scatter(self.h, C.c_int(eb), _ptr(map_), C.c_size_t(map_.numel()), _ptr(src),
                                              _ptr(dst)), "scatter")

    def gather_scatter(self, map_in, map_out, src, dst):
        """dst[map_out[i]] = src[map_in[i]]"""
        self._chk(self.lib.cstone_hip_gather_scatter(self.h, C.c_int(src.element_size()), _ptr(map_in), _ptr(map_out),
                                                     C.c_size_t(map_in.numel()), _ptr(src), _ptr(dst)),
                  "gather_scatter")

    def merge_positions(self, keys_a, keys_b, offset=0):
        """positions (int32 storage) of two sorted key runs in their stable merge, ties: run a first"""
        torch = _torch()
        pa = torch.empty(keys_a.numel(), dtype=torch.int32, device=keys_a.device)
        pb = torch.empty(keys_b.numel(), dtype=torch.int32, device=keys_a.device)
        self._chk(self.lib.cstone_hip_merge_positions(self.h, C.c_int(keys_a.element_size() * 8), _ptr(keys_a),
                                                      C.c_size_t(keys_a.numel()), _ptr(keys_b),
                                                      C.c_size_t(keys_b.numel()), C.c_uint32(offset), _ptr(pa),
                                                      _ptr(pb)), "merge_positions")
        return pa, pb

    def minmax(self, x):
        out = (C.c_double * 2)()
        self._chk(self.lib.cstone_hip_minmax(self.h, C.c_int(x.element_size() * 8), _ptr(x), C.c_size_t(x.numel()),
                                             out), "minmax")
        return out[0], out[1]

    def minmax_arrays(self, arrays):
        """[(min, max), ...] of 1..3 equally long arrays: one launch, one read-back"""
        k = len(arrays)
        out = (C.c_double * (2 * k))()
        ptrs = (C.c_void_p * k)(*[a.data_ptr() for a in arrays])
        self._chk(self.lib.cstone_hip_minmax_arrays(self.h, C.c_int(arrays[0].element_size() * 8), ptrs, C.c_int(k),
                                                    C.c_size_t(arrays[0].numel()), out), "minmax_arrays")
        return [(out[2 * i], out[2 * i + 1]) for i in range(k)]

    def exclusive_scan(self, inp, out, init=0):
        self._chk(self.lib.cstone_hip_exclusive_scan_u32(self.h, _ptr(inp), _ptr(out), C.c_size_t(inp.numel()),
                                                         C.c_uint32(init)), "exclusive_scan")

    def inclusive_scan(self, inp, out):
        self._chk(self.lib.cstone_hip_inclusive_scan_u32(self.h, _ptr(inp), _ptr(out), C.c_size_t(inp.numel())),
                  "inclusive_scan")

    def offsets_from_counts(self, counts, out):
        """out[i] = sum(counts[0..i)) for i <= n (out holds n + 1 values)"""
        assert out.numel() == counts.numel() + 1
        self._chk(self.lib.cstone_hip_offsets_from_counts_u32(self.h, _ptr(counts), _ptr(out), C.c_size_t(counts.numel())),
                  "offsets_from_counts")

    def gather_tables(self, index_map, a, n_a, b, n_b, c, out):
        """out = [a[map[:n_a]] (zeros if a is None), b[map[n_a:n_a + n_b]], c] (uint32 device tensors)"""
        n_c = 0 if c is None else c.numel()
        self._chk(self.lib.cstone_hip_gather_tables_u32(self.h, _ptr(index_map), C.c_void_p(a.data_ptr() if a is not None else 0),
                                                        C.c_size_t(n_a), _ptr(b), C.c_size_t(n_b),
                                                        C.c_void_p(c.data_ptr() if c is not None else 0), C.c_size_t(n_c),
                                                        _ptr(out)), "gather_tables")

    def lower_bound(self, keys, values):
        """positions (int64 device tensor) of the first key >= values[q], unsigned comparison of the bit patterns"""
        torch = _torch()
        out = torch.empty(values.numel(), dtype=torch.int64, device=keys.device)
        self._chk(self.lib.cstone_hip_lower_bound(self.h, C.c_int(keys.element_size() * 8), _ptr(keys),
                                                  C.c_size_t(keys.numel()), _ptr(values), C.c_int(values.numel()),
                                                  _ptr(out)), "lower_bound")
        return out

    # ---- tree
    def compute_node_counts(self, tree, keys, counts=None, max_count=0xFFFFFFFF, num_nodes=None):
        torch = _torch()
        kb = keys.element_size() * 8
        nn = tree.numel() - 1 if num_nodes is None else num_nodes
        if counts is None:
            counts = torch.zeros(nn, dtype=torch.int32, device=tree.device)
        self._chk(self.lib.cstone_hip_compute_node_counts(self.h, C.c_int(kb), _ptr(tree), _ptr(counts), C.c_int(nn),
                                                          _ptr(keys), C.c_size_t(keys.numel()),
                                                          C.c_uint32(max_count)), "compute_node_counts")
        return counts

    def compute_node_counts_guided(self, tree, keys, guess, max_count=0xFFFFFFFF):
        torch = _torch()
        nn = tree.numel() - 1
        counts = torch.zeros(nn, dtype=torch.int32, device=tree.device)
        self._chk(self.lib.cstone_hip_compute_node_counts_guided(self.h, C.c_int(keys.element_size() * 8), _ptr(tree),
                                                                 _ptr(counts), C.c_int(nn), _ptr(keys),
                                                                 C.c_size_t(keys.numel()), C.c_uint32(max_count),
                                                                 _ptr(guess)), "compute_node_counts_guided")
        return counts

    def compute_node_ops(self, tree, counts, bucket, num_nodes=None):
        torch = _torch()
        kb = tree.element_size() * 8
        nn = tree.numel() - 1 if num_nodes is None else num_nodes
        ops = torch.zeros(nn + 1, dtype=torch.int32, device=tree.device)
        new_n, conv = C.c_int(0), C.c_int(0)
        self._chk(self.lib.cstone_hip_compute_node_ops(self.h, C.c_int(kb), _ptr(tree), C.c_int(nn), _ptr(counts),
                                                       C.c_uint32(bucket), _ptr(ops), C.byref(new_n), C.byref(conv)),
                  "compute_node_ops")
        return ops, new_n.value, bool(conv.value)

    def rebalance_tree(self, tree, ops, new_num_nodes, num_nodes=None):
        torch = _torch()
        kb = tree.element_size() * 8
        nn = tree.numel() - 1 if num_nodes is None else num_nodes
        new_tree = torch.zeros(new_num_nodes + 1, dtype=tree.dtype, device=tree.device)
        self._chk(self.lib.cstone_hip_rebalance_tree(self.h, C.c_int(kb), _ptr(tree), C.c_int(nn),
                                                     C.c_int(new_num_nodes), _ptr(ops), _ptr(new_tree)),
                  "rebalance_tree")
        return new_tree

    def update_octree(self, keys, bucket, tree_buf, counts_buf, num_leaves, max_count=0xFFFFFFFF):
        """tree_buf / counts_buf are capacity buffers; returns (num_leaves, converged)"""
        kb = keys.element_size() * 8
        cap = counts_buf.numel()
        assert tree_buf.numel() >= cap + 1
        nl, conv = C.c_int(num_leaves), C.c_int(0)
        rc = self.lib.cstone_hip_update_octree(self.h, C.c_int(kb), _ptr(keys), C.c_size_t(keys.numel()),
                                               C.c_uint32(bucket), _ptr(tree_buf), _ptr(counts_buf), C.byref(nl),
                                               C.c_int(cap), C.c_uint32(max_count), C.byref(conv))
        if rc == -2:
            return -nl.value, False
        self._chk(rc, "update_octree")
        return nl.value, bool(conv.value)

    def compute_octree(self, keys, bucket, cap_leaves=None, max_count=0xFFFFFFFF):
        torch = _torch()
        kb = keys.element_size() * 8
        n = keys.numel()
        cap = cap_leaves or max(4096, 4 * n // max(1, bucket) + 4096)
        while True:
            tree = torch.zeros(cap + 1, dtype=keys.dtype, device=keys.device)
            counts = torch.zeros(cap, dtype=torch.int32, device=keys.device)
            nl, iters = C.c_int(0), C.c_int(0)
            rc = self.lib.cstone_hip_compute_octree(self.h, C.c_int(kb), _ptr(keys), C.c_size_t(n), C.c_uint32(bucket),
                                                    _ptr(tree), _ptr(counts), C.byref(nl), C.c_int(cap),
                                                    C.c_uint32(max_count), C.byref(iters))
            if rc == -2:
                cap = nl.value + 1
                continue
            self._chk(rc, "compute_octree")
            return tree[:nl.value + 1], counts[:nl.value], iters.value

    def build_octree(self, leaves, num_leaves=None):
        torch = _torch()
        kb = leaves.element_size() * 8
        nl = leaves.numel() - 1 if num_leaves is None else num_leaves
        ni = (nl - 1) // 7
        nn = nl + ni
        dev = leaves.device
        o = dict(
            num_leaves=nl, num_internal=ni, num_nodes=nn,
            prefixes=torch.zeros(nn, dtype=leaves.dtype, device=dev),
            child_offsets=torch.zeros(nn + 1, dtype=torch.int32, device=dev),
            parents=torch.zeros(max(1, (nn - 1) // 8), dtype=torch.int32, device=dev),
            level_range=torch.zeros(max_level(kb) + 2, dtype=torch.int32, device=dev),
            internal_to_leaf=torch.zeros(nn, dtype=torch.int32, device=dev),
            leaf_to_internal=torch.zeros(nn, dtype=torch.int32, device=dev),
        )
        self._chk(self.lib.cstone_hip_build_octree(self.h, C.c_int(kb), _ptr(leaves), C.c_int(nl), _ptr(o["prefixes"]),
                                                   _ptr(o["child_offsets"]), _ptr(o["parents"]),
                                                   _ptr(o["level_range"]), _ptr(o["internal_to_leaf"]),
                                                   _ptr(o["leaf_to_internal"])), "build_octree")
        return o

    def upsweep_sum(self, octree, counts):
        self._chk(self.lib.cstone_hip_upsweep_sum(self.h, C.c_int(octree["level_range"].numel()),
                                                  _ptr(octree["level_range"]), _ptr(octree["child_offsets"]),
                                                  _ptr(counts)), "upsweep_sum")

    def node_centers(self, curve, prefixes, box, real_bits=64):
        torch = _torch()
        kb = prefixes.element_size() * 8
        nn = prefixes.numel()
        dt = torch.float32 if real_bits == 32 else torch.float64
        centers = torch.zeros((nn, 3), dtype=dt, device=prefixes.device)
        sizes = torch.zeros((nn, 3), dtype=dt, device=prefixes.device)
        self._chk(self.lib.cstone_hip_node_centers(self.h, C.c_int(curve), C.c_int(kb), C.c_int(real_bits),
                                                   _ptr(prefixes), C.c_int(nn), C.byref(box), _ptr(centers),
                                                   _ptr(sizes)), "node_centers")
        return centers, sizes

    # ---- halos
    def halo_radii(self, h, layout, first, last, num_leaves, ext=1.0):
        torch = _torch()
        radii = torch.empty(num_leaves, dtype=torch.float32, device=h.device)
        self._chk(self.lib.cstone_hip_halo_radii(self.h, C.c_int(h.element_size() * 8), _ptr(h), _ptr(layout),
                                                 C.c_int(first), C.c_int(last), C.c_int(num_leaves), C.c_float(ext),
                                                 _ptr(radii)), "halo_radii")
        return radii

    def find_halos(self, curve, octree, leaves, radii, box, first, last, real_bits=64, flags=None):
        torch = _torch()
        kb = leaves.element_size() * 8
        if flags is None:
            flags = torch.zeros(octree["num_leaves"], dtype=torch.int32, device=leaves.device)
        self._chk(self.lib.cstone_hip_find_halos(self.h, C.c_int(curve), C.c_int(kb), C.c_int(real_bits),
                                                 _ptr(octree["prefixes"]), _ptr(octree["child_offsets"]),
                                                 _ptr(octree["internal_to_leaf"]), _ptr(leaves), _ptr(radii),
                                                 C.byref(box), C.c_int(first), C.c_int(last), _ptr(flags)),
                  "find_halos")
        return flags

    def halo_boxes(self, curve, leaves, radii, box, first, last, real_bits=64):
        torch = _torch()
        kb = leaves.element_size() * 8
        boxes = torch.zeros((last - first, 8), dtype=torch.int32, device=leaves.device)
        self._chk(self.lib.cstone_hip_halo_boxes(self.h, C.c_int(curve), C.c_int(kb), C.c_int(real_bits), _ptr(leaves),
                                                 _ptr(radii), C.byref(box), C.c_int(first), C.c_int(last),
                                                 _ptr(boxes)), "halo_boxes")
        return boxes

    def halo_boxes_foreign(self, curve, octree, leaves, radii, box, first, last, real_bits=64):
        """halo_boxes whose record[6] is set only for boxes that really overlap a leaf outside [first, last)"""
        torch = _torch()
        kb = leaves.element_size() * 8
        boxes = torch.zeros((last - first, 8), dtype=torch.int32, device=leaves.device)
        self._chk(self.lib.cstone_hip_halo_boxes_foreign(
            self.h, C.c_int(curve), C.c_int(kb), C.c_int(real_bits), _ptr(octree["prefixes"]),
            _ptr(octree["child_offsets"]), _ptr(octree["internal_to_leaf"]), _ptr(leaves), _ptr(radii), C.byref(box),
            C.c_int(first), C.c_int(last), _ptr(boxes)), "halo_boxes_foreign")
        return boxes

    def find_overlaps(self, curve, octree, leaves, boxes, first, last, flags=None):
        torch = _torch()
        kb = leaves.element_size() * 8
        if flags is None:
            flags = torch.zeros(octree["num_leaves"], dtype=torch.int32, device=leaves.device)
        nb = boxes.shape[0] if boxes.dim() == 2 else boxes.numel() // 8
        self._chk(self.lib.cstone_hip_find_overlaps(self.h, C.c_int(curve), C.c_int(kb), _ptr(octree["prefixes"]),
                                                    _ptr(octree["child_offsets"]), _ptr(octree["internal_to_leaf"]),
                                                    _ptr(leaves), _ptr(boxes), C.c_int(nb), C.c_int(first),
                                                    C.c_int(last), _ptr(flags)), "find_overlaps")
        return flags

    def find_neighbors(self, x, y, z, h, first, last, box, octree, layout, centers, sizes, ngmax, ext=1.0):
        torch = _torch()
        nw = last - first
        nidx = torch.zeros((nw, ngmax), dtype=torch.int32, device=x.device)
        nc = torch.zeros(nw, dtype=torch.int32, device=x.device)
        self._chk(self.lib.cstone_hip_find_neighbors(self.h, C.c_int(x.element_size() * 8), _ptr(x), _ptr(y), _ptr(z),
                                                     _ptr(h), C.c_uint32(first), C.c_uint32(last), C.byref(box),
                                                     _ptr(octree["child_offsets"]), _ptr(octree["internal_to_leaf"]),
                                                     _ptr(layout), _ptr(centers), _ptr(sizes), C.c_float(ext),
                                                     C.c_uint32(ngmax), _ptr(nidx), _ptr(nc)), "find_neighbors")
        return nidx, nc

    def adapt_smoothing_lengths(self, x, y, z, h, first, last, box, octree, layout, centers, sizes, ng0, tol, max_iter,
                                grow_limit=float("inf"), ngmax=0):
        """cstone_hip_adapt_smoothing_lengths: h[first:last] iterated IN PLACE to ng0 +- tol neighbours (the rule: include/
        cstone_hip.h).  Returns (neighbors [last - first, ngmax] or None if ngmax == 0, counts, status), status = walks |
        ADAPT_H_* flags.  Rows of neighbors beyond min(count, ngmax) are not written (they are zero here)"""
        torch = _torch()
        if h.dtype != x.dtype:
            raise ValueError("h must have the coordinates' type")
        nw = last - first
        nidx = torch.zeros((nw, ngmax), dtype=torch.int32, device=x.device) if ngmax else None
        nc = torch.zeros(nw, dtype=torch.int32, device=x.device)
        st = torch.zeros(nw, dtype=torch.int32, device=x.device)
        self._chk(self.lib.cstone_hip_adapt_smoothing_lengths(
            self.h, C.c_int(x.element_size() * 8), _ptr(x), _ptr(y), _ptr(z), _ptr(h), C.c_uint32(first),
            C.c_uint32(last), C.byref(box), _ptr(octree["child_offsets"]), _ptr(octree["internal_to_leaf"]), _ptr(layout),
            _ptr(centers), _ptr(sizes), C.c_uint32(ng0), C.c_uint32(tol), C.c_uint32(max_iter), C.c_float(grow_limit),
            C.c_uint32(ngmax), _ptr(nidx), _ptr(nc), _ptr(st)), "adapt_smoothing_lengths")
        return nidx, nc, st

    def friends_of_friends(self, x, y, z, first, last, box, octree, layout, centers, sizes, linking_length,
                           want_sizes=True, want_num_groups=True):
        """cstone_hip_friends_of_friends: (labels [last - first], group sizes or None, number of groups or None); labels hold
        the lowest particle index of each particle's group (the rule: include/cstone_hip.h).  Asking for the number of
        groups synchronises the stream"""
        torch = _torch()
        nw = last - first
        labels = torch.zeros(nw, dtype=torch.int32, device=x.device)
        gs = torch.zeros(nw, dtype=torch.int32, device=x.device) if want_sizes else None
        ng = C.c_uint32(0)
        self._chk(self.lib.cstone_hip_friends_of_friends(
            self.h, C.c_int(x.element_size() * 8), _ptr(x), _ptr(y), _ptr(z), C.c_uint32(first), C.c_uint32(last),
            C.byref(box), _ptr(octree["child_offsets"]), _ptr(octree["internal_to_leaf"]), _ptr(layout), _ptr(centers),
            _ptr(sizes), C.c_double(linking_length), _ptr(labels), _ptr(gs),
            C.byref(ng) if want_num_groups else None), "friends_of_friends")
        return labels, gs, (ng.value if want_num_groups else None)

    def fof_lower_labels(self, component, labels, changed, first=0, last=None):
        """cstone_hip_fof_lower_labels, the device step of a round of friends-of-friends across ranks: labels (int64
        tensor holding uint64 bits, IN PLACE) get the minimum over the entries with the same component (int32 tensor,
        values in [0, n)); changed (int32 tensor of one element) grows by the labels of [first, last) that dropped.
        Asynchronous"""
        n = labels.numel()
        self._chk(self.lib.cstone_hip_fof_lower_labels(self.h, _ptr(component), n, first, n if last is None else last,
                                                       _ptr(labels), _ptr(changed)), "fof_lower_labels")

    def fof_catalog(self, labels, first, last, min_members=1, capacity=None):
        """cstone_hip_fof_catalog: (group_offsets [num_groups + 1], members [number of particles listed]) of the groups with
        at least min_members members, by ascending label, members ascending"""
        torch = _torch()
        nw = last - first
        cap = nw + 1 if capacity is None else capacity
        offsets = torch.zeros(max(cap, 1), dtype=torch.int32, device=labels.device)
        members = torch.zeros(max(nw, 1), dtype=torch.int32, device=labels.device)
        ng = C.c_uint32(0)
        self._chk(self.lib.cstone_hip_fof_catalog(self.h, _ptr(labels), C.c_uint32(first), C.c_uint32(last),
                                                  C.c_uint32(min_members), _ptr(offsets), C.c_size_t(cap), _ptr(members),
                                                  C.byref(ng)), "fof_catalog")
        offsets = offsets[:ng.value + 1]
        return offsets, members[:int(offsets[-1].item())]

    def fof_group_properties(self, x, y, z, m, group_offsets, members, box, vel=None, want_radius=True, want_flags=True):
        """cstone_hip_fof_group_properties on a catalogue as fof_catalog returns it: (mass [G], center [G, 3], velocity
        [G, 3] or None, radius [G] or None, flags [G] (int32 holding the CSTONE_FOF_GROUP_* bits) or None) in the
        coordinate type.  vel: (vx, vy, vz) or None.  The rule: include/cstone_hip.h.  Asynchronous"""
        torch = _torch()
        ng = group_offsets.numel() - 1
        mass = torch.zeros(ng, dtype=x.dtype, device=x.device)
        center = torch.zeros((ng, 3), dtype=x.dtype, device=x.device)
        velocity = torch.zeros((ng, 3), dtype=x.dtype, device=x.device) if vel is not None else None
        radius = torch.zeros(ng, dtype=x.dtype, device=x.device) if want_radius else None
        flags = torch.zeros(ng, dtype=torch.int32, device=x.device) if want_flags else None
        vx, vy, vz = vel if vel is not None else (None, None, None)
        self._chk(self.lib.cstone_hip_fof_group_properties(
            self.h, x.element_size() * 8, m.element_size() * 8, _ptr(x), _ptr(y), _ptr(z), _ptr(m), _ptr(vx), _ptr(vy),
            _ptr(vz), C.cast(C.byref(box), C.c_void_p), _ptr(group_offsets), _ptr(members), ng, _ptr(mass), _ptr(center),
            _ptr(velocity), _ptr(radius), _ptr(flags)), "fof_group_properties")
        return mass, center, velocity, radius, flags

    def sphere_profiles(self, x, y, z, w, first, last, box, octree, layout, centers, sizes, query_centers, edges,
                        query_scale=None, num_queries=None, counts=None, sums=None, flags=None, real_bits=None,
                        mass_bits=None):
        """cstone_hip_sphere_profiles: for every query centre (query_centers [Q, 3], the coordinates' type) the particles
        of [first, last) counted, and their weights w (float32 / float64 tensor or None) summed in float64, in the
        half-open distance bins [s * edges[b], s * edges[b + 1]), s = query_scale[q] (or 1).  edges: NB + 1 host numbers.
        Returns (counts [Q, NB] int64, sums [Q, NB] float64 or None without w, flags [Q] int32 holding SPHERE_TOO_WIDE).
        The rule: include/cstone_hip.h.  counts, sums, flags: tensors to write into instead of new ones; num_queries,
        real_bits, mass_bits: overrides of what the tensors imply.  Asynchronous"""
        torch = _torch()
        e, nb = sphere_edges(edges)
        nq = query_centers.shape[0] if num_queries is None else num_queries
        dev = query_centers.device
        rows = (nq, max(nb, 0))
        if counts is None:
            counts = torch.zeros(rows, dtype=torch.int64, device=dev)
        if sums is None and w is not None:
            sums = torch.zeros(rows, dtype=torch.float64, device=dev)
        if flags is None:
            flags = torch.zeros(nq, dtype=torch.int32, device=dev)
        rb = query_centers.element_size() * 8 if real_bits is None else real_bits
        mb = (w.element_size() * 8 if w is not None else 64) if mass_bits is None else mass_bits
        self._chk(self.lib.cstone_hip_sphere_profiles(
            self.h, rb, mb, _opt(x), _opt(y), _opt(z), _opt(w), first, last, C.cast(C.byref(box), C.c_void_p),
            _opt(octree["child_offsets"]), _opt(octree["internal_to_leaf"]), _opt(layout), _opt(centers), _opt(sizes),
            _opt(query_centers), _opt(query_scale), nq, e, nb, _opt(counts), _opt(sums), _opt(flags)), "sphere_profiles")
        return counts, sums, flags

    def pair_counts(self, x, y, z, w, first, last, box, octree, layout, centers, sizes, edges, t_first=None, t_last=None,
                    counts=None, sums=None, with_stats=False, real_bits=None, w_bits=None):
        """cstone_hip_pair_counts: the ORDERED pairs (i, j), i in [t_first, t_last) (default: [first, last)), j in
        [first, last), j != i by index, counted in the half-open distance bins [edges[b], edges[b + 1]), and the products
        of their weights w (float32 / float64 tensor or None) summed in float64.  edges: NB + 1 host numbers.  Returns
        (counts [NB] int64, sums [NB] float64 or None without w, stats): stats is None, or with_stats a pair (distance
        tests issued, pairs binned) -- the call then synchronises.  The rule: include/cstone_hip.h.  counts, sums: tensors
        to write into instead of new ones; real_bits, w_bits: overrides of what the tensors imply"""
        torch = _torch()
        e, nb = sphere_edges(edges)
        t_first = first if t_first is None else t_first
        t_last = last if t_last is None else t_last
        if counts is None:
            counts = torch.zeros(max(nb, 0), dtype=torch.int64, device=self.device)
        if sums is None and w is not None:
            sums = torch.zeros(max(nb, 0), dtype=torch.float64, device=self.device)
        rb = x.element_size() * 8 if real_bits is None else real_bits
        wb = (w.element_size() * 8 if w is not None else 64) if w_bits is None else w_bits
        st = (C.c_uint64 * 2)() if with_stats else None
        self._chk(self.lib.cstone_hip_pair_counts(
            self.h, rb, wb, _opt(x), _opt(y), _opt(z), _opt(w), first, last, t_first, t_last,
            C.cast(C.byref(box), C.c_void_p), _opt(octree["child_offsets"]), _opt(octree["internal_to_leaf"]), _opt(layout),
            _opt(centers), _opt(sizes), e, nb, _opt(counts), _opt(sums), st), "pair_counts")
        return counts, sums, (int(st[0]), int(st[1])) if with_stats else None

    def pair_counts_cross(self, x, y, z, w, first, last, box, octree, layout, centers, sizes, query_centers, edges,
                          query_w=None, num_queries=None, counts=None, sums=None, with_stats=False, real_bits=None,
                          w_bits=None):
        """cstone_hip_pair_counts_cross: every pair (query, particle of [first, last)) binned like pair_counts, nothing
        excluded; query_centers [Q, 3] in the coordinates' type, in any order; query_w [Q] (the type of w) or None for 1.
        Returns (counts [NB] int64, sums [NB] float64 or None without w, stats)"""
        torch = _torch()
        e, nb = sphere_edges(edges)
        nq = query_centers.shape[0] if num_queries is None else num_queries
        if counts is None:
            counts = torch.zeros(max(nb, 0), dtype=torch.int64, device=self.device)
        if sums is None and w is not None:
            sums = torch.zeros(max(nb, 0), dtype=torch.float64, device=self.device)
        rb = query_centers.element_size() * 8 if real_bits is None else real_bits
        wb = (w.element_size() * 8 if w is not None else 64) if w_bits is None else w_bits
        st = (C.c_uint64 * 2)() if with_stats else None
        self._chk(self.lib.cstone_hip_pair_counts_cross(
            self.h, rb, wb, _opt(x), _opt(y), _opt(z), _opt(w), first, last, C.cast(C.byref(box), C.c_void_p),
            _opt(octree["child_offsets"]), _opt(octree["internal_to_leaf"]), _opt(layout), _opt(centers), _opt(sizes),
            _opt(query_centers), _opt(query_w), nq, e, nb, _opt(counts), _opt(sums), st), "pair_counts_cross")
        return counts, sums, (int(st[0]), int(st[1])) if with_stats else None

    def knn(self, x, y, z, first, last, box, octree, layout, centers, sizes, query_centers, k, query_rmax=None,
            query_self=None, num_queries=None, neighbors=None, dist2=None, counts=None, with_dist2=True, with_counts=True,
            real_bits=None):
        """cstone_hip_knn: for every query centre (query_centers [Q, 3], the coordinates' type) the k nearest particles
        of [first, last), ordered by (squared distance, index).  query_rmax [Q] (or None): only particles with
        d2 < rmax * rmax; query_self [Q] int32 (or None): one index per query that is left out, KNN_NONE for none.
        Returns (neighbors [Q, k] int32 holding absolute indices, dist2 [Q, k] in the coordinates' type, counts [Q]
        int32); unfilled slots hold -1 (KNN_NONE) and +inf.  with_dist2 / with_counts = False pass NULL and return None
        there.  neighbors, dist2, counts: tensors to write into instead of new ones; num_queries, real_bits: overrides of
        what the tensors imply.  The rule: include/cstone_hip.h.  Asynchronous"""
        torch = _torch()
        nq = query_centers.shape[0] if num_queries is None else num_queries
        dev = query_centers.device
        cols = min(max(int(k), 0), KNN_MAX_K)
        if neighbors is None:
            neighbors = torch.full((nq, cols), -1, dtype=torch.int32, device=dev)
        if dist2 is None and with_dist2:
            dist2 = torch.full((nq, cols), float("inf"), dtype=query_centers.dtype, device=dev)
        if counts is None and with_counts:
            counts = torch.zeros(nq, dtype=torch.int32, device=dev)
        rb = query_centers.element_size() * 8 if real_bits is None else real_bits
        self._chk(self.lib.cstone_hip_knn(
            self.h, rb, _opt(x), _opt(y), _opt(z), first, last, C.cast(C.byref(box), C.c_void_p),
            _opt(octree["child_offsets"]), _opt(octree["internal_to_leaf"]), _opt(layout), _opt(centers), _opt(sizes),
            _opt(query_centers), _opt(query_rmax), _opt(query_self), nq, k, _opt(neighbors), _opt(dist2), _opt(counts)),
            "knn")
        return neighbors, dist2, counts

    def spherical_overdensity(self, sums, edges, rho_threshold, query_scale=None, profile_flags=None, real_bits=64,
                              num_queries=None, r_delta=None, m_delta=None, flags=None):
        """cstone_hip_spherical_overdensity: (R_Delta [Q], M_Delta [Q], flags [Q]) from the sums [Q, NB] of a
        sphere_profiles call with the same edges (edges[0] must be 0) and scales: the radius where the mean enclosed
        density falls to rho_threshold, interpolated between the bin edges, and the mass inside; flags hold
        SPHERE_TOO_WIDE (passed on), SO_NOT_REACHED, SO_UNRESOLVED.  real_bits: the type of query_scale.  Asynchronous"""
        torch = _torch()
        e, nb = sphere_edges(edges)
        nq = sums.shape[0] if num_queries is None else num_queries
        if query_scale is not None:
            real_bits = query_scale.element_size() * 8
        if r_delta is None:
            r_delta = torch.zeros(nq, dtype=torch.float64, device=sums.device)
        if m_delta is None:
            m_delta = torch.zeros(nq, dtype=torch.float64, device=sums.device)
        if flags is None:
            flags = torch.zeros(nq, dtype=torch.int32, device=sums.device)
        self._chk(self.lib.cstone_hip_spherical_overdensity(
            self.h, real_bits, _opt(query_scale), nq, e, nb, _opt(sums), _opt(profile_flags), float(rho_threshold),
            _opt(r_delta), _opt(m_delta), _opt(flags)), "spherical_overdensity")
        return r_delta, m_delta, flags

    def compute_fixed_groups(self, first, last, group_size):
        torch = _torch()
        cap = (last - first + group_size - 1) // max(group_size, 1) + 1
        groups = torch.zeros(cap, dtype=torch.int32, device=self.device)
        ng = C.c_uint32(0)
        self._chk(self.lib.cstone_hip_compute_fixed_groups(self.h, C.c_uint32(first), C.c_uint32(last),
                                                           C.c_uint32(group_size), _ptr(groups), C.byref(ng)),
                  "compute_fixed_groups")
        return groups[:ng.value + 1]

    def compute_group_splits(self, first, last, x, y, z, leaves, layout, box, group_size, tol_factor, capacity=None):
        """groups[num_groups + 1]: groupStart = groups[:-1], groupEnd = groups[1:]"""
        torch = _torch()
        cap = last - first + 1 if capacity is None else capacity
        groups = torch.zeros(max(cap, 1), dtype=torch.int32, device=self.device)
        ng = C.c_uint32(0)
        self._chk(self.lib.cstone_hip_compute_group_splits(
            self.h, C.c_int(leaves.element_size() * 8), C.c_int(x.element_size() * 8), C.c_uint32(first),
            C.c_uint32(last), _ptr(x), _ptr(y), _ptr(z), _ptr(leaves), C.c_int(leaves.numel() - 1), _ptr(layout),
            C.byref(box), C.c_uint32(group_size), C.c_float(tol_factor), _ptr(groups), C.c_size_t(cap), C.byref(ng)),
            "compute_group_splits")
        return groups[:ng.value + 1]

    def find_neighbors_groups(self, x, y, z, h, first, last, groups, box, octree, layout, centers, sizes, ngmax,
                              ext=1.0):
        torch = _torch()
        nw = last - first
        nidx = torch.zeros((nw, ngmax), dtype=torch.int32, device=x.device)
        nc = torch.zeros(nw, dtype=torch.int32, device=x.device)
        ng = groups.numel() - 1
        self._chk(self.lib.cstone_hip_find_neighbors_groups(
            self.h, C.c_int(x.element_size() * 8), _ptr(x), _ptr(y), _ptr(z), _ptr(h), C.c_uint32(first),
            C.c_uint32(last), _ptr(groups), C.c_void_p(groups.data_ptr() + 4), C.c_uint32(ng), C.byref(box),
            _ptr(octree["child_offsets"]), _ptr(octree["internal_to_leaf"]), _ptr(layout), _ptr(centers), _ptr(sizes),
            C.c_float(ext), C.c_uint32(ngmax), _ptr(nidx), _ptr(nc)), "find_neighbors_groups")
        return nidx, nc

    # ---- gravity
    def upsweep_multipoles(self, x, y, z, m, leaf_to_internal, layout, level_range, child_offsets, expansion_centers,
                           multipoles=None):
        """multipoles (num_nodes, 8) = (M, Qxx, Qxy, Qxz, Qyy, Qyz, Qzz, 0) about the expansion centres (num_nodes, 4);
        leaf_to_internal: the LEAF part of the map (num_leaves = layout.numel() - 1 entries), level_range: the level
        ranges of the linked octree (host sequence or tensor, every level that exists)"""
        torch = _torch()
        nn = expansion_centers.numel() // 4
        levels = np.ascontiguousarray(np.asarray(level_range.cpu() if hasattr(level_range, "cpu") else level_range,
                                                 dtype=np.int32))
        if multipoles is None:
            multipoles = torch.zeros((nn, 8), dtype=x.dtype, device=x.device)
        self._chk(self.lib.cstone_hip_upsweep_multipoles(
            self.h, C.c_int(x.element_size() * 8), C.c_int(m.element_size() * 8), _ptr(x), _ptr(y), _ptr(z), _ptr(m),
            _ptr(leaf_to_internal), C.c_int(layout.numel() - 1), _ptr(layout), C.c_int(levels.size - 1),
            levels.ctypes.data_as(C.c_void_p), _ptr(child_offsets), C.c_int(nn), _ptr(expansion_centers),
            _ptr(multipoles)), "upsweep_multipoles")
        return multipoles

    def compute_gravity(self, x, y, z, m, first, last, groups, box, child_offsets, internal_to_leaf, layout,
                        expansion_centers, multipoles, order=2, G=1.0, eps2=0.0, potential=True, counts=False, h=None):
        """(ax, ay, az, phi, p2p_counts, m2p_counts) of the targets [first, last) (phi None unless potential, the counts
        None unless counts); groups: num_groups + 1 indices as compute_group_splits returns them; h: per-particle
        softening lengths laid out like x (cstone_hip_compute_gravity_h), None: Plummer softening with eps2 alone"""
        torch = _torch()
        nt = last - first

        def out(dt):
            return torch.zeros(nt, dtype=dt, device=x.device)

        ax, ay, az = out(x.dtype), out(x.dtype), out(x.dtype)
        phi = out(x.dtype) if potential else None
        p2p, m2p = (out(torch.int32), out(torch.int32)) if counts else (None, None)
        head = (self.h, C.c_int(x.element_size() * 8), C.c_int(m.element_size() * 8), _ptr(x), _ptr(y), _ptr(z), _ptr(m))
        tail = (C.c_uint32(first), C.c_uint32(last), _ptr(groups), C.c_uint32(groups.numel() - 1), C.byref(box),
                _ptr(child_offsets), _ptr(internal_to_leaf), _ptr(layout), _ptr(expansion_centers), _ptr(multipoles),
                C.c_int(order), C.c_double(G), C.c_double(eps2), _ptr(ax), _ptr(ay), _ptr(az), _ptr(phi), _ptr(p2p),
                _ptr(m2p))
        if h is None:
            self._chk(self.lib.cstone_hip_compute_gravity(*head, *tail), "compute_gravity")
        else:
            self._check_h(x, h)
            self._chk(self.lib.cstone_hip_compute_gravity_h(*head, _ptr(h), *tail), "compute_gravity_h")
        return ax, ay, az, phi, p2p, m2p

    @staticmethod
    def _check_h(x, h):
        if h.dtype != x.dtype or h.numel() < x.numel():
            raise CstoneError("h must have the type of the coordinates and an element for every particle")

    def compute_gravity_let(self, x, y, z, m, first, last, groups, box, child_offsets, internal_to_leaf, layout,
                            expansion_centers, multipoles, order=2, G=1.0, eps2=0.0, potential=True, counts=False,
                            h=None):
        """compute_gravity on a locally essential tree (cstone_hip_compute_gravity_let): an opened leaf WITHOUT particles
        is applied as a multipole.  Returns (ax, ay, az, phi, p2p_counts, m2p_counts, let_m2p_counts), the last one the
        number of such leaves per target (they are counted in m2p_counts too).  h: as in compute_gravity"""
        torch = _torch()
        nt = last - first

        def out(dt):
            return torch.zeros(nt, dtype=dt, device=x.device)

        ax, ay, az = out(x.dtype), out(x.dtype), out(x.dtype)
        phi = out(x.dtype) if potential else None
        p2p, m2p, let = (out(torch.int32), out(torch.int32), out(torch.int32)) if counts else (None, None, None)
        head = (self.h, C.c_int(x.element_size() * 8), C.c_int(m.element_size() * 8), _ptr(x), _ptr(y), _ptr(z), _ptr(m))
        tail = (C.c_uint32(first), C.c_uint32(last), _ptr(groups), C.c_uint32(groups.numel() - 1), C.byref(box),
                _ptr(child_offsets), _ptr(internal_to_leaf), _ptr(layout), _ptr(expansion_centers), _ptr(multipoles),
                C.c_int(order), C.c_double(G), C.c_double(eps2), _ptr(ax), _ptr(ay), _ptr(az), _ptr(phi), _ptr(p2p),
                _ptr(m2p), _ptr(let))
        if h is None:
            self._chk(self.lib.cstone_hip_compute_gravity_let(*head, *tail), "compute_gravity_let")
        else:
            self._check_h(x, h)
            self._chk(self.lib.cstone_hip_compute_gravity_let_h(*head, _ptr(h), *tail), "compute_gravity_let_h")
        return ax, ay, az, phi, p2p, m2p, let

    @staticmethod
    def _host_levels(level_range):
        return np.ascontiguousarray(np.asarray(level_range.cpu() if hasattr(level_range, "cpu") else level_range,
                                               dtype=np.int32))

    def upsweep_octupoles(self, x, y, z, m, leaf_to_internal, layout, level_range, child_offsets, expansion_centers,
                          multipoles, octupoles=None):
        """octupoles (num_nodes, 8) = (Oxxx, Oxxy, Oxxz, Oxyy, Oxyz, Oyyy, Oyyz, 0) about the expansion centres
        (cstone_hip_upsweep_octupoles); multipoles: the result of upsweep_multipoles for the same tree and centres (read,
        not written); the other arguments as for upsweep_multipoles"""
        torch = _torch()
        nn = expansion_centers.numel() // 4
        levels = self._host_levels(level_range)
        if octupoles is None:
            octupoles = torch.zeros((nn, 8), dtype=x.dtype, device=x.device)
        self._chk(self.lib.cstone_hip_upsweep_octupoles(
            self.h, C.c_int(x.element_size() * 8), C.c_int(m.element_size() * 8), _ptr(x), _ptr(y), _ptr(z), _ptr(m),
            _ptr(leaf_to_internal), C.c_int(layout.numel() - 1), _ptr(layout), C.c_int(levels.size - 1),
            levels.ctypes.data_as(C.c_void_p), _ptr(child_offsets), C.c_int(nn), _ptr(expansion_centers),
            _ptr(multipoles), _ptr(octupoles)), "upsweep_octupoles")
        return octupoles

    def upsweep_octupoles_nodes(self, level_range, child_offsets, expansion_centers, multipoles, octupoles):
        """the internal-node part of upsweep_octupoles alone (cstone_hip_upsweep_octupoles_nodes): octupoles, whose leaf
        rows are filled, gets its internal rows in place and is returned"""
        nn = expansion_centers.numel() // 4
        levels = self._host_levels(level_range)
        self._chk(self.lib.cstone_hip_upsweep_octupoles_nodes(
            self.h, C.c_int(octupoles.element_size() * 8), C.c_int(levels.size - 1), levels.ctypes.data_as(C.c_void_p),
            _ptr(child_offsets), C.c_int(nn), _ptr(expansion_centers), _ptr(multipoles), _ptr(octupoles)),
            "upsweep_octupoles_nodes")
        return octupoles

    def compute_gravity_o3(self, x, y, z, m, first, last, groups, box, child_offsets, internal_to_leaf, layout,
                           expansion_centers, multipoles, octupoles, let=False, G=1.0, eps2=0.0, potential=True,
                           counts=False, h=None):
        """the walk at order 3 (cstone_hip_compute_gravity_o3): compute_gravity (let False) or compute_gravity_let (let
        True) with the octupole term.  Returns (ax, ay, az, phi, p2p_counts, m2p_counts), and let_m2p_counts as a seventh
        if let; h: as in compute_gravity"""
        torch = _torch()
        nt = last - first

        def out(dt):
            return torch.zeros(nt, dtype=dt, device=x.device)

        ax, ay, az = out(x.dtype), out(x.dtype), out(x.dtype)
        phi = out(x.dtype) if potential else None
        p2p, m2p = (out(torch.int32), out(torch.int32)) if counts else (None, None)
        letc = out(torch.int32) if counts and let else None
        if h is not None:
            self._check_h(x, h)
        self._chk(self.lib.cstone_hip_compute_gravity_o3(
            self.h, C.c_int(x.element_size() * 8), C.c_int(m.element_size() * 8), _ptr(x), _ptr(y), _ptr(z), _ptr(m),
            _ptr(h), C.c_uint32(first), C.c_uint32(last), _ptr(groups), C.c_uint32(groups.numel() - 1), C.byref(box),
            _ptr(child_offsets), _ptr(internal_to_leaf), _ptr(layout), _ptr(expansion_centers), _ptr(multipoles),
            _ptr(octupoles), C.c_int(1 if let else 0), C.c_double(G), C.c_double(eps2), _ptr(ax), _ptr(ay), _ptr(az),
            _ptr(phi), _ptr(p2p), _ptr(m2p), _ptr(letc)), "compute_gravity_o3")
        return (ax, ay, az, phi, p2p, m2p, letc) if let else (ax, ay, az, phi, p2p, m2p)

    def direct_gravity(self, x, y, z, m, h=None, first=0, last=None, targets=None, num_segments=0, G=1.0, eps2=0.0,
                       potential=True):
        """all-pairs direct sum (cstone_hip_direct_gravity): (ax, ay, az, phi) of every source [0, n) on the targets
        [first, last) (last None: n) or, if targets (int32 tensor of particle indices, any order, duplicates allowed) is
        given, on those; outputs indexed by target position.  h: per-particle softening lengths or None;
        num_segments: how many pieces the sources are cut into (0: the library chooses)"""
        torch = _torch()
        n = x.numel()
        last = n if last is None else last
        if h is not None:
            self._check_h(x, h)
        if targets is not None and targets.dtype != torch.int32:
            raise CstoneError("targets must be an int32 tensor (u32 bit patterns)")
        nt = targets.numel() if targets is not None else max(0, last - first)
        ax, ay, az = [torch.zeros(nt, dtype=x.dtype, device=x.device) for _ in range(3)]
        phi = torch.zeros(nt, dtype=x.dtype, device=x.device) if potential else None
        self._chk(self.lib.cstone_hip_direct_gravity(
            self.h, C.c_int(x.element_size() * 8), C.c_int(m.element_size() * 8), _ptr(x), _ptr(y), _ptr(z), _ptr(m),
            _ptr(h), C.c_uint32(n), C.c_uint32(first), C.c_uint32(last), _ptr(targets),
            C.c_uint32(targets.numel() if targets is not None else 0), C.c_int(num_segments), C.c_double(G),
            C.c_double(eps2), _ptr(ax), _ptr(ay), _ptr(az), _ptr(phi)), "direct_gravity")
        return ax, ay, az, phi


_DEFAULT = None


def load(device=0):
    """shared default context (tests)"""
    global _DEFAULT
    if _DEFAULT is None:
        _DEFAULT = Context(device)
    return _DEFAULT
