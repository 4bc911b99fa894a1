"""The device scans (csrc/scan.hip behind cstone_hip_exclusive_scan_u32, _inclusive_scan_u32, _offsets_from_counts_u32,
and the 64-bit cstone_hip_scan_u32_to_u64 of csrc/primitives.hip) against tree_support.scan_model, bit for bit: at the
tile counts where scanJobs changes its path (1024 tiles of 2048 elements: two launches up to there, three beyond), where
the tile-sum loops of blockScanKernel<false> (256-wide strides) and scanSumsKernel (256-wide chunks) start a new round,
with sums that wrap modulo 2^32, in place, on views that are only 4-byte aligned -- and many calls of different sizes
back to back on one context with no output read in between, the pattern of a domain sync.

Two backends with one body (let_ops_support): `cpu` (no marker) checks the model against the CPU restatement of the ABI,
`hip` (@gpu) lets the model judge the kernels."""
import ctypes as C

import numpy as np
import pytest

import let_ops_support as S
import tree_support as T

gpu = pytest.mark.gpu
TILE = 2048
SIZES = [0, 1, 7, 8, 9, 2047, 2048, 2049,
         # blockScanKernel<false> adds up the tile sums before its own in strides of 256 (t = lane; t < blockIdx.x):
         # up to 257 tiles one round for every workgroup; the last workgroup of 258 tiles is the first with a second
         # round, that of 514 tiles the first with a third
         256 * TILE - 1, 256 * TILE, 256 * TILE + 1, 257 * TILE + 1,
         512 * TILE - 1, 512 * TILE, 512 * TILE + 1, 513 * TILE + 1,
         1024 * TILE - 1, 1024 * TILE, 1024 * TILE + 1,  # the last size with two launches, the first with three
         1025 * TILE + 1,
         1281 * TILE + 5,                                 # scanSumsKernel: the sixth chunk of 256 tile sums holds two
         5000003]
SENTINEL = 0xC0FFEE11


@pytest.fixture(params=["cpu", pytest.param("hip", marks=gpu)])
def be(request):
    if request.param == "cpu":
        return S.cpu_backend()
    return S.HipBackend(request.getfixturevalue("hip"))


class Scans:
    """the four entries on device buffers; offsets count ELEMENTS into the buffers"""

    def __init__(self, be):
        self.be, self.lib, self.ctx = be, be.lib, be.ctx

    def exclusive(self, src, dst, n, init=0, src_at=0, dst_at=0):
        self.be.chk(self.lib.cstone_hip_exclusive_scan_u32(self.ctx, self.be.ptr(src, 4 * src_at), self.be.ptr(dst, 4 * dst_at),
                                                           C.c_size_t(n), C.c_uint32(init)), "exclusive_scan_u32")

    def inclusive(self, src, dst, n, src_at=0, dst_at=0):
        self.be.chk(self.lib.cstone_hip_inclusive_scan_u32(self.ctx, self.be.ptr(src, 4 * src_at), self.be.ptr(dst, 4 * dst_at),
                                                           C.c_size_t(n)), "inclusive_scan_u32")

    def offsets(self, src, dst, n, dst_at=0):
        self.be.chk(self.lib.cstone_hip_offsets_from_counts_u32(self.ctx, self.be.ptr(src), self.be.ptr(dst, 4 * dst_at),
                                                                C.c_size_t(n)), "offsets_from_counts_u32")

    def to_u64(self, src, dst, n, init, inclusive):
        self.be.chk(self.lib.cstone_hip_scan_u32_to_u64(self.ctx, self.be.ptr(src), self.be.ptr(dst), C.c_size_t(n),
                                                        C.c_uint64(init), C.c_int(inclusive)), "scan_u32_to_u64")


def values(kind, n):
    if kind == "ones":  # the result is an iota: any tile out of order shows
        return np.ones(n, np.uint32)
    if kind == "zeros":
        return np.zeros(n, np.uint32)
    if kind == "full-range":  # sums wrap modulo 2^32 within a few elements
        return np.random.default_rng(n + 1).integers(0, 1 << 32, n, dtype=np.uint32)
    v = np.zeros(n, np.uint32)  # "spikes": a single non-zero in the last slot of a tile and in the first of the next
    for tile in (1, 256, 1024, n // TILE):
        for at, x in ((tile * TILE - 1, 0xFFFFFFF0), (tile * TILE, 0x25)):
            if 0 <= at < n:
                v[at] = x
    return v


KINDS = ("ones", "zeros", "full-range", "spikes")


@pytest.mark.parametrize("n", SIZES)
def test_every_form_at_every_size(be, n):
    sc = Scans(be)
    for kind, init in zip(KINDS, (0, 5, T.U32_MAX, 5)):
        v = values(kind, n)
        ex, inc = T.scan_model(v, init), T.scan_model(v, 0, inclusive=True)
        src = be.to_dev(v)
        out = be.filled(n, np.uint32, SENTINEL)
        sc.exclusive(src, out, n, init)
        assert np.array_equal(be.to_host(out, np.uint32), ex), (kind, "exclusive")
        out = be.filled(n, np.uint32, SENTINEL)
        sc.inclusive(src, out, n)
        assert np.array_equal(be.to_host(out, np.uint32), inc), (kind, "inclusive")
        # in place: the form of every tree update
        both = be.to_dev(v)
        sc.exclusive(both, both, n, init)
        assert np.array_equal(be.to_host(both, np.uint32), ex), (kind, "exclusive in place")
        both = be.to_dev(v)
        sc.inclusive(both, both, n)
        assert np.array_equal(be.to_host(both, np.uint32), inc), (kind, "inclusive in place")
        assert np.array_equal(be.to_host(src, np.uint32), v)
        # n + 1 offsets between two sentinels
        out = be.filled(n + 3, np.uint32, SENTINEL)
        sc.offsets(src, out, n, dst_at=1)
        got = be.to_host(out, np.uint32)
        assert got[0] == SENTINEL and got[n + 2] == SENTINEL and np.array_equal(got[1:n + 2], T.offsets_model(v)), kind
        # 64-bit sums of the 32-bit values
        for inclusive, init64 in ((0, 0), (1, (1 << 40) + 3)):
            out = be.filled(n + 1, np.uint64, SENTINEL)
            sc.to_u64(src, out, n, init64, inclusive)
            got = be.to_host(out, np.uint64)
            assert got[n] == SENTINEL and np.array_equal(got[:n], T.scan_model(v, init64, bool(inclusive), bits=64)), kind
    if n >= 2048:
        assert int(T.scan_model(values("full-range", n), 0, True, bits=64)[-1]) > 1 << 32  # (the 64-bit sums pass 2^32)


@pytest.mark.parametrize("n", [9, 2049, 256 * TILE + 1, 1024 * TILE + 1])
def test_views_one_and_three_elements_into_an_allocation(be, n):
    """nothing but 4-byte alignment may be assumed of in and out; what lies around the view stays"""
    sc = Scans(be)
    v = values("full-range", n + 8)
    for src_at, dst_at in ((1, 3), (3, 1), (1, 1)):
        src = be.to_dev(v)
        want = np.full(n + 8, SENTINEL, np.uint32)
        out = be.to_dev(want)
        sc.exclusive(src, out, n, 5, src_at, dst_at)
        want[dst_at:dst_at + n] = T.scan_model(v[src_at:src_at + n], 5)
        assert np.array_equal(be.to_host(out, np.uint32), want)
        want[dst_at:dst_at + n] = T.scan_model(v[src_at:src_at + n], 0, True)
        sc.inclusive(src, out, n, src_at, dst_at)
        assert np.array_equal(be.to_host(out, np.uint32), want)
        # in place on the view
        want = v.copy()
        want[src_at:src_at + n] = T.scan_model(v[src_at:src_at + n], 0)
        sc.exclusive(src, src, n, 0, src_at, src_at)
        assert np.array_equal(be.to_host(src, np.uint32), want)


# the sizes of one pass, large and small in turn; the form of call i is FORMS[i % 5]
BACK_TO_BACK = [1024 * TILE + 1, 9, 256 * TILE, 1, 5000003, 2049, 1025 * TILE + 1, 0, 512 * TILE + 1, 2047,
                1024 * TILE, 8, 1281 * TILE + 5, 2048, 256 * TILE + 1, 7, 1024 * TILE - 1, 255, 512 * TILE - 1, 65,
                1024 * TILE + 1, 3, 5000003, 4097, 256 * TILE - 1, 1, 1025 * TILE + 1, 2049, 512 * TILE, 9,
                1024 * TILE, 63, 1281 * TILE + 5, 2048, 1024 * TILE + 1, 64, 300000, 7, 1024 * TILE - 1, 100]
FORMS = ("exclusive in place", "inclusive", "offsets", "exclusive", "inclusive in place")


def issue_back_to_back(be, order):
    """every call of the pass -> [(what, expected, output buffer)], nothing fetched.  Everything the calls need is on
    the device before the first one: inputs, output buffers, the tree and the counts and ops buffers of the
    decisions; between the sync in front of the loop and its end there are ABI calls only.  The scans enqueue their
    launches and return; compute_node_ops hands two host scalars back and therefore waits for the stream itself,
    which is part of its contract."""
    sc, api = Scans(be), T.Api(be, 64)
    tree = T.uniform(64, 3)
    dtree = api.dev(tree)
    inputs = {}
    for n in set(BACK_TO_BACK):
        v = values("full-range", n)
        inputs[n] = (v, be.to_dev(v))
    counts = [np.random.default_rng(i).choice(np.array([0, 16, 17, 200], np.uint32), 512) for i in range(8)]
    dcounts = [api.dev(c) for c in counts]
    plan = []  # (what, form, n, source, output, expected)
    for at, i in enumerate(order):
        n, form = BACK_TO_BACK[i], FORMS[i % 5]
        v, src = inputs[n]
        if form == "exclusive in place":
            out, want = be.to_dev(v), T.scan_model(v, 0)
        elif form == "inclusive in place":
            out, want = be.to_dev(v), T.scan_model(v, 0, True)
        elif form == "inclusive":
            out, want = be.filled(n, np.uint32, SENTINEL), T.scan_model(v, 0, True)
        elif form == "offsets":
            out, want = be.filled(n + 1, np.uint32, SENTINEL), T.offsets_model(v)
        else:
            out, want = be.filled(n, np.uint32, SENTINEL), T.scan_model(v, i)
        plan.append((f"call {at}: {form} of {n}", form, n, i, src, out, want))
        if at % 5 == 4:  # the decisions of a small tree: the same arena, the same device scalars
            k = (at // 5) % 8
            model, model_conv = T.ops_model(tree, counts[k], 16)
            ops = be.filled(tree.size, np.uint32, SENTINEL)
            plan.append((f"node_ops after call {at}", "node_ops", (int(model.sum()), int(model_conv)), i, dcounts[k], ops,
                         T.scan_model(model)))
    be.sync()
    scalars = []
    for what, form, n, i, src, out, want in plan:  # ABI calls only
        if form == "exclusive in place":
            sc.exclusive(out, out, n, 0)
        elif form == "inclusive in place":
            sc.inclusive(out, out, n)
        elif form == "inclusive":
            sc.inclusive(src, out, n)
        elif form == "offsets":
            sc.offsets(src, out, n)
        elif form == "exclusive":
            sc.exclusive(src, out, n, i)
        else:
            scalars.append((what, n, api.node_ops(dtree, src, 16, ops=out)[1:]))
    for what, want, got in scalars:
        assert got == want, what
    return [(what, want, out) for what, _, _, _, _, out, want in plan]


@pytest.mark.parametrize("direction", ["forward", "reversed"])
def test_forty_scans_back_to_back_on_one_context(be, direction):
    """one pass of about forty scans of mixed size and form with the decisions of a small tree in between, no output
    read before the last call is issued (the scans do not wait for the stream; compute_node_ops, which returns host
    scalars, does); then every output against the model"""
    order = list(range(len(BACK_TO_BACK)))
    pending = issue_back_to_back(be, order if direction == "forward" else order[::-1])
    for what, want, out in pending:
        assert np.array_equal(be.to_host(out, np.uint32)[:want.size], want), what
