"""The streaming and seam primitives of csrc/primitives.hip and csrc/extras.hip, each entry point of include/cstone_hip.h
called ON ITS OWN through ctypes and compared with `==` / np.array_equal against a numpy model written from the contract
comment in that header (the models and the case builders: tests/primitives_support.py).  No tolerance anywhere; no NaN
in any input.

Covered: minmax, minmax_arrays, count_equal, reduce_sum, increment, max_norm_square, scale, segment_max, gather_ranges,
lower_bound_value, fill, gather, scatter, gather_scatter, gather_multi -- every compiled element width, type and index
width, at 1 / 255 / 256 / 257 / 1023 / 1024 / 1025 elements and at the sizes, derived from the device's number of compute
units, at which a grid-stride kernel takes a second step or the min/max kernel enters its four-loads-deep loop.

Unmarked tests check the case builders against their own premises (a planted extreme is the unique extreme and lies in
the loop region it is named after, a sum really passes 2^32 / wraps 2^64, ...).  The entries that the CPU restatement of
the ABI serves (gather, scatter, gather_scatter, fill, count_equal, gather_ranges with 32-bit indices) run the same body
on the `cpu` backend of tests/let_ops_support.py, which judges the model without a GPU."""
import ctypes as C

import numpy as np
import pytest

import let_ops_support as S
import primitives_support as P

gpu = pytest.mark.gpu
PAD = 0x5A


@pytest.fixture(params=["cpu", pytest.param("hip", marks=gpu)])
def be(request):
    if request.param == "cpu":
        return S.cpu_backend()
    return S.HipBackend(request.getfixturevalue("hip"))


@pytest.fixture
def dev(hip):
    return S.HipBackend(hip)


def num_cu(be):
    """the number ctx->numCu holds; the cpu backend has no strides, any number serves"""
    if be.name == "cpu":
        return 64
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def typed(buf, dtype):
    """torch view of a device allocation of the hip backend, to change single elements in place"""
    import torch

    return buf.raw[:buf.nbytes].view({np.float32: torch.float32, np.float64: torch.float64}[dtype])


def rows(be, buf, width):
    return be.to_host(buf, np.uint8).reshape(-1, width)


# ----------------------------------------------------------------------------------------------------------------------
# the builders against their premises (no GPU)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", P.CU_COUNTS)
@pytest.mark.parametrize("itemsize", [4, 8])
def test_minmax_plants_lie_in_the_loop_they_are_named_after(cus, itemsize):
    sizes = P.minmax_sizes(itemsize, cus)
    vec = 16 // itemsize
    assert sizes["one_trip"] == vec * 8 * 256 * cus + 1
    assert sizes["four_deep"] == vec * (3 * 8 * 256 * cus) + 4 * vec * 256 + 3
    for name, n in sizes.items():
        for offset in (0, 1, 3):
            part, trip = P.minmax_reader(n, offset, itemsize, cus)
            plants = P.minmax_plants(n, offset, itemsize, cus)
            assert part.size == n
            four, single = np.nonzero(part == P.FOUR)[0], np.nonzero(part == P.SINGLE)[0]
            assert plants["first"] == 0 and plants["last"] == n - 1
            assert part[0] == (P.HEAD if offset % vec else P.FOUR if name == "four_deep" else P.SINGLE)
            if "head_last" in plants:
                assert part[plants["head_last"]] == P.HEAD and part[plants["head_last"] + 1] != P.HEAD
            if "tail_first" in plants:
                assert part[plants["tail_first"]] == P.TAIL and part[plants["tail_first"] - 1] != P.TAIL
            if name == "four_deep":
                head, npk, _, stride = P.minmax_layout(n, offset, itemsize, cus)
                assert stride == 8 * 256 * cus and 1024 <= npk - 3 * stride <= 1025
                assert four.size == 4 * vec * (npk - 3 * stride) and single.size == 3 * vec * (4 * stride - npk)
                assert plants["four_first"] == four[0] and plants["four_last"] == four[-1]
                # the fourth load of the deep step is the only reader of everything behind the three-stride mark
                k3 = plants["four_last_load_first"]
                assert (part[k3:four[-1] + 1] == P.FOUR).all() and part[k3 - 1] == P.SINGLE
                assert plants["single_first"] == single[0] and plants["single_last"] == single[-1]
                assert (trip[four] == 0).all() and set(trip[single]) == {0, 1, 2}
                if offset == 0:  # the scalar tail the issue's size leaves behind aligned packs
                    assert (part == P.TAIL).sum() == 3 % vec and part[n - 1] == P.TAIL
            elif name == "second_trip":
                assert four.size == 0 and trip[plants["trip2_first"]] == 1 and trip[plants["trip1_last"]] == 0
                assert trip[plants["trip2_first"] - 1] == 0 and plants["trip2_first"] == plants["trip1_last"] + 1
            else:
                assert four.size == 0 and (trip == 0).all()  # every lane reads one pack: the size the issue names
    for n in P.EDGE_SIZES:
        part, _ = P.minmax_reader(n, 1, itemsize, cus)
        assert part.size == n and not (part == P.FOUR).any()


def test_planted_extremes_are_the_unique_extremes():
    rng = np.random.default_rng(1)
    for dtype in (np.float32, np.float64):
        a = P.noise(rng, 200001, dtype)
        assert a.dtype == dtype and (np.abs(a) < 1).all()
        assert (np.abs(P.noise(rng, 1000, dtype, 100.0)) < 100).all()
        lo, hi = a.min(), a.max()
        for pos in (0, 77, int(a.argmin()), int(a.argmax()), a.size - 1):
            for value in (-1e6, 1e6):
                b = a.copy()
                b[pos] = value
                assert P.extremes_with(a, lo, hi, {pos: value}) == [float(b.min()), float(b.max())]
                assert (b == dtype(value)).sum() == 1 and (b.min() == dtype(value) or b.max() == dtype(value))
        b = a.copy()
        b[3], b[9] = -2e6, 3e6
        assert P.extremes_with(a, lo, hi, {3: -2e6, 9: 3e6}) == [-2e6, 3e6] == [float(b.min()), float(b.max())]
        one = a[:1]
        assert P.extremes_with(one, one[0], one[0], {0: 1e6}) == [1e6, 1e6]


@pytest.mark.parametrize("cus", P.CU_COUNTS)
def test_reduction_cases_meet_their_premises(cus):
    rng = np.random.default_rng(2)
    n = P.count_big(cus)
    s = P.stride_of(n, 8, cus)
    assert s == 8 * 256 * cus and 2 * s < n  # a third step for the first 77 lanes
    for bits in (32, 64):
        for size in (1, 2, 64, 257, n):
            cases = {name: (data, init) for name, data, init in P.sum_cases(rng, bits, size)}
            data = cases["near_top"][0]
            assert data.dtype == P.uint(bits) and data.size == size
            if bits == 32:
                assert size < 2 or P.exact_sum(data[:2]) > 1 << 32  # passes 2^32 within the first wave
                assert P.exact_sum(data) == sum(int(v) for v in data[:5000]) + P.exact_sum(data[5000:])
                if size == n:  # 2^52 on a part of 256 compute units
                    assert (n << 32) - (n << 20) <= P.exact_sum(data) < n << 32 and (cus < 256 or n << 31 > 1 << 51)
                assert P.reduce_sum_model(*cases["init_near_2^63"]) > 1 << 63
            else:
                assert size < 2 or P.exact_sum(data) >= 1 << 64  # wraps
                assert P.reduce_sum_model(data, 5) == (5 + sum(int(v) for v in data[:300]) + P.exact_sum(data[300:])) % (1 << 64)
            assert cases["init_wraps"][1] + P.exact_sum(data) >= 1 << 64
            last = cases["only_last"][0]
            assert np.count_nonzero(last) == 1 and last[-1] != 0
        for name, data, value in P.count_cases(rng, bits, n, cus):
            hits = np.nonzero(data == P.uint(bits)(value))[0]
            if name == "last_only":
                assert list(hits) == [n - 1]
            elif name == "second_stride_only":
                assert hits.size == 3 and hits.min() >= s
            elif name == "nowhere":
                assert hits.size == 0
            elif name == "everywhere":
                assert hits.size == n
            elif name == "low_word_matches":
                low = (data & np.uint64(0xFFFFFFFF)) == np.uint64(value & 0xFFFFFFFF)
                assert 0 < hits.size < n // 50 and low.sum() > n // 2
            else:
                assert 0 < hits.size < n
        assert "second_stride_only" not in [c[0] for c in P.count_cases(rng, bits, 1025, cus)]
        for name, data, value in P.increment_cases(rng, bits, 1025):
            want = P.increment_model(data, value)
            assert [int(w) for w in want[:50]] == [(int(d) + value % (1 << bits)) % (1 << bits) for d in data[:50]]
            assert (want < data).any() and (want > data).any()  # some elements wrap, some do not
    m = P.norm_big(cus)
    s4 = P.stride_of(m, 4, cus)
    plants = P.norm_plants(m, cus)
    assert plants["stride2"] // s4 == 1 and plants["stride3"] // s4 == 2 and plants["last"] == m - 1
    for w in range(4):
        i = plants[f"last_group_wave{w}"]
        assert i // 256 == 4 * cus - 1 and (i % 256) // 64 == w
    for size in P.EDGE_SIZES:
        for name, i in P.norm_plants(size, cus).items():
            assert 0 <= i < size and not name.startswith("stride")
            if name.startswith("last_group"):
                assert i // 256 == (size - 1) // 256 and (i % 256) // 64 == int(name[-1])


def test_segment_cases_meet_their_premises():
    rng = np.random.default_rng(3)
    lists = P.segment_length_lists(rng)
    firsts = {lengths[0] for name, lengths in lists if name.startswith("rotation")}
    lasts = {lengths[-1] for name, lengths in lists if name.startswith("rotation")}
    assert firsts == lasts == set(P.SEGMENT_LENGTHS)
    for name, lengths in lists:
        if name.startswith("rotation"):
            assert sorted(lengths) == sorted(list(P.SEGMENT_LENGTHS) + [0, 0, 0])
            assert any(lengths[i:i + 3] == [0, 0, 0] for i in range(1, len(lengths) - 3))
    assert sorted(len(lengths) for name, lengths in lists if name.startswith("count")) == sorted(P.SEGMENT_COUNTS)
    assert [len(lengths) for name, lengths in lists if name == "random5000"] == [5000]
    lanes = set()
    for name, lengths in lists:
        for ib in (32, 64):
            off = P.segment_offsets(lengths, 64)
            pos, at = P.segment_values(rng, lengths, "positive", ib)
            neg, _ = P.segment_values(rng, lengths, "negative", ib)
            mix, _ = P.segment_values(rng, lengths, "mixed", ib)
            assert pos.size == off[-1] + 3 and off[0] == 5 and (pos[:5] == 1e9).all() and (pos[-3:] == 1e9).all()
            inner = slice(5, int(off[-1]))
            assert (pos[inner] > 0).all() and (neg[inner] < 0).all() and (mix[inner] > 0).any() and (mix[inner] < 0).any()
            for s, ln in enumerate(lengths):
                seg = pos[int(off[s]):int(off[s + 1])]
                if ln:
                    assert int(seg.argmax()) == at[s] and (seg == seg.max()).sum() == 1 and seg.max() > 1
                    lanes.add(int(at[s]))
            if ib == 64:
                assert (pos[inner].astype(np.float32).astype(np.float64) != pos[inner]).mean() > 0.9  # not floats
            want = P.segment_max_model(mix, off, 64)
            assert (want[::3] == 0).all() and (want > 0).any()
            assert (P.segment_max_model(neg, off, 32) == 0).all()
    assert lanes >= set(range(17))


def test_range_cases_hold_the_empty_range_placements():
    rng = np.random.default_rng(4)
    nsrc = 170000
    for ib in (32, 64):
        for size in P.EDGE_SIZES + (100003,):
            (_, scan, off), (_, one_scan, one_off) = P.range_cases(rng, size, nsrc, ib)
            ln = np.diff(scan.astype(np.int64))
            assert scan.dtype == off.dtype == P.uint(ib) and scan[0] == 0 and scan[-1] == size and off.size == ln.size
            assert list(ln[:2]) == [0, 0] and list(ln[-2:]) == [0, 0]
            assert any(list(ln[i:i + 3]) == [0, 0, 0] for i in range(2, ln.size - 4)) or size == 1
            full = np.nonzero(ln)[0]
            assert full.size == min(size, 7) and (off.astype(np.int64) + ln <= nsrc).all()
            if full.size >= 3:
                a, b, c = full[:3]
                assert int(off[b]) == int(off[a]) + ln[a]  # touches
                assert int(off[b]) <= int(off[c]) <= int(off[b]) + ln[b]  # overlaps
                if size > 1000:
                    assert int(off[c]) < int(off[b]) + ln[b]
            if ib == 64:
                assert (off > 1 << 16).all() and one_off[0] > 1 << 16
            assert list(one_scan) == [0, size] and one_off.size == 1
            src = np.arange(nsrc, dtype=np.int64)
            want = P.gather_ranges_model(scan, off, src)
            assert np.array_equal(want, S.range_indices(off, scan))


def test_lower_bound_cases_hold_what_they_are_named_after():
    rng = np.random.default_rng(5)
    for kind, dt in P.LOWER_BOUND_KINDS.items():
        names = set()
        for n in P.LOWER_BOUND_SIZES:
            for a, values in P.lower_bound_cases(rng, kind, n):
                assert a.dtype == dt and a.size == n and (a[1:] >= a[:-1]).all()
                for name, v in values:
                    names.add(name)
                    at = P.lower_bound_model(a, v)
                    assert type(v) is dt
                    if name == "below":
                        assert at == 0
                    elif name == "above":
                        assert at == n or (kind == 4 and np.isinf(a[-1]) and a[at] == np.inf and a[at - 1] < np.inf)
                    elif name == "present_once":
                        assert a[at] == v and (a == v).sum() == 1
                    elif name == "first_of_run":
                        assert a[at] == v and (a == v).sum() > 1 and (at == 0 or a[at - 1] < v)
                    elif name == "absent":
                        assert 0 < at < n and a[at - 1] < v < a[at]
                if kind == 4:
                    assert not np.isnan(a).any()
                    tiny = np.float32(1e-42)
                    assert 0 < tiny < np.finfo(np.float32).tiny
                elif n == 5000:
                    info = np.iinfo(dt)
                    assert int(a[0]) < info.min // 2 + info.max // 2 < int(a[-1])  # both halves of the type
                    assert kind in (0, 1) or a[0] < 0
        assert names >= {"below", "above", "present_once", "first_of_run", "absent"}


# ----------------------------------------------------------------------------------------------------------------------
# 1. minmax, minmax_arrays
# ----------------------------------------------------------------------------------------------------------------------
def call_minmax(be, bits, buf, offset, n):
    out = (C.c_double * 2)(7.0, 7.0)
    be.chk(be.lib.cstone_hip_minmax(be.ctx, C.c_int(bits), be.ptr(buf, offset * bits // 8), C.c_size_t(n), out), "minmax")
    return list(out)


@gpu
@pytest.mark.parametrize("bits", [32, 64])
def test_minmax(dev, bits):
    """every edge size and the three stride-crossing sizes, at two alignments; at each, plain noise and then one planted
    extreme (+-1e6) at a time at every place minmax_plants names"""
    be, dtype, cus = dev, P.real(bits), num_cu(dev)
    rng = np.random.default_rng(10 + bits)
    sizes = P.minmax_sizes(bits // 8, cus)
    base = P.noise(rng, max(sizes.values()) + 4, dtype)
    buf = be.to_dev(base)
    t = typed(buf, dtype)
    for n in P.EDGE_SIZES + tuple(sizes.values()):
        for offset in (0, 1):
            view = base[offset:offset + n]
            lo, hi = view.min(), view.max()
            assert call_minmax(be, bits, buf, offset, n) == [float(lo), float(hi)], (n, offset)
            for name, pos in P.minmax_plants(n, offset, bits // 8, cus).items():
                for value in (-1e6, 1e6):
                    t[offset + pos] = value
                    got = call_minmax(be, bits, buf, offset, n)
                    t[offset + pos] = float(view[pos])
                    assert got == P.extremes_with(view, lo, hi, {pos: value}), (n, offset, name, value)
    assert np.array_equal(be.to_host(buf, dtype), base)


def call_minmax_arrays(be, bits, bufs, offsets, n):
    k = len(bufs)
    ptrs = (C.c_void_p * k)(*[be.ptr(b, o * bits // 8).value for b, o in zip(bufs, offsets)])
    out = (C.c_double * 8)(*([7.0] * 8))
    be.chk(be.lib.cstone_hip_minmax_arrays(be.ctx, C.c_int(bits), ptrs, C.c_int(k), C.c_size_t(n), out), "minmax_arrays")
    assert list(out)[2 * k:] == [7.0] * (8 - 2 * k)
    return list(out)[:2 * k]


@gpu
@pytest.mark.parametrize("bits", [32, 64])
def test_minmax_arrays(dev, bits):
    """1, 2 and 3 arrays that start 0, 1 and 3 elements behind a 16-byte boundary, noise of different scale in each; in
    every round each array gets its minimum and its maximum at two places of its own, of a magnitude of its own"""
    be, dtype, cus = dev, P.real(bits), num_cu(dev)
    rng = np.random.default_rng(20 + bits)
    sizes = P.minmax_sizes(bits // 8, cus)
    offsets = (0, 1, 3)
    base = [P.noise(rng, max(sizes.values()) + 4, dtype, 10.0 ** a) for a in range(3)]
    bufs = [be.to_dev(b) for b in base]
    ts = [typed(b, dtype) for b in bufs]
    for n in P.EDGE_SIZES + tuple(sizes.values()):
        views = [base[a][offsets[a]:offsets[a] + n] for a in range(3)]
        ext = [(v.min(), v.max()) for v in views]
        places = [list(P.minmax_plants(n, offsets[a], bits // 8, cus).values()) for a in range(3)]
        for k in (1, 2, 3):
            plain = call_minmax_arrays(be, bits, bufs[:k], offsets[:k], n)
            assert plain == [float(e) for a in range(k) for e in ext[a]], (n, k)
            for r in range(max(len(p) for p in places)):
                want = []
                for a in range(k):
                    at_min, at_max = places[a][(r + a) % len(places[a])], places[a][(r + a + 1) % len(places[a])]
                    planted = {at_min: -1e6 * (a + 1)}
                    if at_max != at_min:
                        planted[at_max] = 3e6 * (a + 1)
                    for i, v in planted.items():
                        ts[a][offsets[a] + i] = v
                    want += P.extremes_with(views[a], ext[a][0], ext[a][1], planted)
                got = call_minmax_arrays(be, bits, bufs[:k], offsets[:k], n)
                for a in range(k):
                    for i in (places[a][(r + a) % len(places[a])], places[a][(r + a + 1) % len(places[a])]):
                        ts[a][offsets[a] + i] = float(views[a][i])
                assert got == want, (n, k, r)
    for a in range(3):
        assert np.array_equal(be.to_host(bufs[a], dtype), base[a])
    # arrays of one value: that value twice
    value = dtype(0.3)
    same = be.to_dev(np.full(sizes["one_trip"] + 4, value, dtype))
    for n in P.EDGE_SIZES + (sizes["one_trip"],):
        for k in (1, 2, 3):
            assert call_minmax_arrays(be, bits, [same] * k, offsets[:k], n) == [float(value)] * (2 * k), (n, k)


# ----------------------------------------------------------------------------------------------------------------------
# 2. count_equal, reduce_sum, increment
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_count_equal(be, bits):
    cus = num_cu(be)
    rng = np.random.default_rng(30 + bits)
    for n in P.EDGE_SIZES + (P.count_big(cus),):
        for name, data, value in P.count_cases(rng, bits, n, cus):
            got, ddata = C.c_uint64(99), be.to_dev(data)
            be.chk(be.lib.cstone_hip_count_equal(be.ctx, C.c_int(bits), be.ptr(ddata), C.c_size_t(n),
                                                 C.c_uint64(value), C.byref(got)), "count_equal")
            assert got.value == int((data == data.dtype.type(value)).sum()), (n, name)


@gpu
@pytest.mark.parametrize("bits", [32, 64])
def test_reduce_sum(dev, bits):
    be, cus = dev, num_cu(dev)
    rng = np.random.default_rng(40 + bits)
    for n in P.EDGE_SIZES + (P.count_big(cus),):
        for name, data, init in P.sum_cases(rng, bits, n):
            got, ddata = C.c_uint64(99), be.to_dev(data)
            be.chk(be.lib.cstone_hip_reduce_sum(be.ctx, C.c_int(bits), be.ptr(ddata), C.c_size_t(n),
                                                C.c_uint64(init), C.byref(got)), "reduce_sum")
            assert got.value == P.reduce_sum_model(data, init), (n, name)


@gpu
@pytest.mark.parametrize("bits", [32, 64])
def test_increment(dev, bits):
    be, cus = dev, num_cu(dev)
    rng = np.random.default_rng(50 + bits)
    dt = P.uint(bits)
    for n in P.EDGE_SIZES + (P.count_big(cus),):
        for name, data, value in P.increment_cases(rng, bits, n):
            din, dout = be.to_dev(data), be.filled(n + 3, dt, 0x5A5A5A5A)
            be.chk(be.lib.cstone_hip_increment(be.ctx, C.c_int(bits), be.ptr(din), be.ptr(dout), C.c_size_t(n),
                                               C.c_uint64(value)), "increment")
            got = be.to_host(dout, dt)
            assert np.array_equal(got[:n], P.increment_model(data, value)), (n, name)
            assert (got[n:] == 0x5A5A5A5A).all() and np.array_equal(be.to_host(din, dt), data), (n, name)
        be.chk(be.lib.cstone_hip_increment(be.ctx, C.c_int(bits), be.ptr(din), be.ptr(din), C.c_size_t(n), C.c_uint64(3)),
               "increment in place")
        assert np.array_equal(be.to_host(din, dt), P.increment_model(data, 3)), n


# ----------------------------------------------------------------------------------------------------------------------
# 3. max_norm_square, scale
# ----------------------------------------------------------------------------------------------------------------------
def call_norm(be, bits, bufs, n):
    out = C.c_double(-1.0)
    be.chk(be.lib.cstone_hip_max_norm_square(be.ctx, C.c_int(bits), be.ptr(bufs[0]), be.ptr(bufs[1]), be.ptr(bufs[2]),
                                             C.c_size_t(n), C.byref(out)), "max_norm_square")
    return out.value


@gpu
@pytest.mark.parametrize("bits", [32, 64])
def test_max_norm_square(dev, bits):
    """noise, then one vector far above it at a time at every place norm_plants names: a full vector whose squares are
    inexact (so the order of the additions and a fused multiply-add would show) and one with a single component"""
    be, dtype, cus = dev, P.real(bits), num_cu(dev)
    rng = np.random.default_rng(60 + bits)
    vectors = [(123.456, -78.9, 45.67), (0.0, 0.0, 77.7), (-77.7, 0.0, 0.0), (0.0, 3.3, 0.0)]
    for n in P.EDGE_SIZES + (P.norm_big(cus),):
        xyz = [P.noise(rng, n, dtype) for _ in range(3)]
        bufs = [be.to_dev(a) for a in xyz]
        ts = [typed(b, dtype) for b in bufs]
        assert call_norm(be, bits, bufs, n) == P.norm_model(*xyz), n
        for j, (name, pos) in enumerate(P.norm_plants(n, cus).items()):
            for vec in (vectors[0], vectors[1 + j % 3]):
                planted = [dtype(c) for c in vec]
                for t, c in zip(ts, planted):
                    t[pos] = float(c)
                got = call_norm(be, bits, bufs, n)
                for t, a in zip(ts, xyz):
                    t[pos] = float(a[pos])
                want = float((planted[0] * planted[0] + planted[1] * planted[1]) + planted[2] * planted[2])
                assert want > 3 and got == want, (n, name, vec)
        zero = be.to_dev(np.zeros(n, dtype))
        assert call_norm(be, bits, [zero] * 3, n) == 0.0
        for axis in range(3):  # one component carries everything
            only = [zero] * 3
            only[axis] = bufs[axis]
            assert call_norm(be, bits, only, n) == float((xyz[axis] * xyz[axis]).max()), (n, axis)


@gpu
@pytest.mark.parametrize("bits", [32, 64])
def test_scale(dev, bits):
    be, dtype = dev, P.real(bits)
    rng = np.random.default_rng(70 + bits)
    for n in P.EDGE_SIZES + (4097,):
        for factor in (0.3, -2.5e-3, 1e10):
            data = P.noise(rng, n + 5, dtype, 1e3)
            buf = be.to_dev(data)
            be.chk(be.lib.cstone_hip_scale(be.ctx, C.c_int(bits), be.ptr(buf, 2 * bits // 8), C.c_size_t(n),
                                           C.c_double(factor)), "scale")
            want = data.copy()
            want[2:2 + n] = data[2:2 + n] * dtype(factor)
            assert np.array_equal(be.to_host(buf, dtype), want), (n, factor)


# ----------------------------------------------------------------------------------------------------------------------
# 4. segment_max
# ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("index_bits", [32, 64])
@pytest.mark.parametrize("in_bits,out_bits", [(32, 32), (64, 32), (64, 64)])
def test_segment_max(dev, in_bits, out_bits, index_bits):
    be = dev
    rng = np.random.default_rng(80)
    for name, lengths in P.segment_length_lists(rng):
        off = P.segment_offsets(lengths, index_bits)
        doff = be.to_dev(off)
        ns = len(lengths)
        for kind in ("positive", "negative", "mixed"):
            values, _ = P.segment_values(rng, lengths, kind, in_bits)
            out, dval = be.filled(ns + 3, P.real(out_bits), 7.0), be.to_dev(values)
            be.chk(be.lib.cstone_hip_segment_max(be.ctx, C.c_int(in_bits), C.c_int(out_bits), C.c_int(index_bits),
                                                 be.ptr(dval), be.ptr(doff), C.c_size_t(ns), be.ptr(out)),
                   "segment_max")
            got = be.to_host(out, P.real(out_bits))
            want = P.segment_max_model(values, off, out_bits)
            assert np.array_equal(got[:ns], want) and (got[ns:] == 7.0).all(), (name, kind)
            if kind == "negative":
                assert (got[:ns] == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# 5. gather_ranges
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend,index_bits", [("cpu", 32), pytest.param("hip", 32, marks=gpu),
                                                pytest.param("hip", 64, marks=gpu)])
@pytest.mark.parametrize("width", P.RANGE_WIDTHS)
def test_gather_ranges(request, backend, index_bits, width):
    be = S.cpu_backend() if backend == "cpu" else S.HipBackend(request.getfixturevalue("hip"))
    rng = np.random.default_rng(90 + width)
    nsrc = 170000
    src = P.bit_patterns(rng, nsrc, width)
    dsrc = be.to_dev(src)
    for size in P.EDGE_SIZES + (100003,):
        for name, scan, off in P.range_cases(rng, size, nsrc, index_bits):
            buf, dscan, doff = be.filled((size + 3) * width, np.uint8, PAD), be.to_dev(scan), be.to_dev(off)
            be.chk(be.lib.cstone_hip_gather_ranges(be.ctx, C.c_int(width), C.c_int(index_bits), be.ptr(dscan),
                                                   be.ptr(doff), C.c_int(off.size), be.ptr(dsrc), be.ptr(buf),
                                                   C.c_size_t(size)), "gather_ranges")
            got = rows(be, buf, width)
            assert np.array_equal(got[:size], P.gather_ranges_model(scan, off, src)), (size, name)
            assert (got[size:] == PAD).all(), (size, name)


# ----------------------------------------------------------------------------------------------------------------------
# 6. lower_bound_value
# ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", sorted(P.LOWER_BOUND_KINDS))
def test_lower_bound_value(dev, kind):
    be = dev
    rng = np.random.default_rng(100 + kind)
    ctype = {0: C.c_uint32, 1: C.c_uint64, 2: C.c_int32, 3: C.c_int64, 4: C.c_float}[kind]
    for n in P.LOWER_BOUND_SIZES:
        for a, values in P.lower_bound_cases(rng, kind, n):
            da = be.to_dev(a)
            for name, v in values:
                value, got = ctype(v.item()), C.c_uint64(99)
                be.chk(be.lib.cstone_hip_lower_bound_value(be.ctx, C.c_int(kind), be.ptr(da), C.c_size_t(n),
                                                           C.byref(value), C.byref(got)), "lower_bound_value")
                assert got.value == P.lower_bound_model(a, v), (n, name, v)


# ----------------------------------------------------------------------------------------------------------------------
# 7. fill
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 4, 8])
def test_fill(be, width):
    value = bytes([0xC3, 0x01, 0xFE, 0x80, 0x7F, 0x10, 0xAA, 0x55][:width])
    for n in P.EDGE_SIZES:
        buf = be.filled((n + 8) * width, np.uint8, PAD)
        be.chk(be.lib.cstone_hip_fill(be.ctx, C.c_int(width), be.ptr(buf, 3 * width), C.c_size_t(n), value), "fill")
        got = rows(be, buf, width)
        assert (got[:3] == PAD).all() and (got[3 + n:] == PAD).all(), n
        assert (got[3:3 + n] == np.frombuffer(value, np.uint8)).all(), n
    if be.name == "hip":
        for bad in (2, 16):
            buf = be.filled(64, np.uint8, PAD)
            assert be.lib.cstone_hip_fill(be.ctx, C.c_int(bad), be.ptr(buf), C.c_size_t(2), bytes(16)) == S.E_ARG
            assert (be.to_host(buf, np.uint8) == PAD).all()


# ----------------------------------------------------------------------------------------------------------------------
# 8. gather, scatter, gather_scatter, gather_multi
# ----------------------------------------------------------------------------------------------------------------------
FRONT = 2  # elements in front of a destination sub-view


@pytest.mark.parametrize("width", P.PERMUTE_WIDTHS)
def test_gather(be, width):
    rng = np.random.default_rng(110 + width)
    for n in P.PERMUTE_SIZES:
        nsrc = n + 37
        src = P.bit_patterns(rng, nsrc, width)
        dsrc = be.to_dev(src)
        for name, map_ in P.gather_maps(rng, n, nsrc):
            dst, dmap = be.filled((FRONT + n + 3) * width, np.uint8, PAD), be.to_dev(map_)
            be.chk(be.lib.cstone_hip_gather(be.ctx, C.c_int(width), be.ptr(dmap), C.c_size_t(n), be.ptr(dsrc),
                                            be.ptr(dst, FRONT * width)), "gather")
            got = rows(be, dst, width)
            assert np.array_equal(got[FRONT:FRONT + n], P.gather_model(map_, src)), (n, name)
            assert (got[:FRONT] == PAD).all() and (got[FRONT + n:] == PAD).all(), (n, name)


@pytest.mark.parametrize("width", P.PERMUTE_WIDTHS)
def test_scatter(be, width):
    rng = np.random.default_rng(120 + width)
    for n in P.PERMUTE_SIZES:
        src = P.bit_patterns(rng, n, width)
        map_ = rng.permutation(n).astype(np.uint32)
        dst, dmap, dsrc = be.filled((FRONT + n + 3) * width, np.uint8, PAD), be.to_dev(map_), be.to_dev(src)
        be.chk(be.lib.cstone_hip_scatter(be.ctx, C.c_int(width), be.ptr(dmap), C.c_size_t(n), be.ptr(dsrc),
                                         be.ptr(dst, FRONT * width)), "scatter")
        got = rows(be, dst, width)
        want = P.scatter_model(map_, src, np.full((n, width), PAD, np.uint8))
        assert np.array_equal(got[FRONT:FRONT + n], want), n
        assert (got[:FRONT] == PAD).all() and (got[FRONT + n:] == PAD).all(), n
        # half of the elements, to every second place: the places in between stay
        half = (n + 1) // 2
        dst = be.filled((n + 3) * width, np.uint8, PAD)
        sparse = (2 * rng.permutation(half)).astype(np.uint32)
        dmap = be.to_dev(sparse)
        be.chk(be.lib.cstone_hip_scatter(be.ctx, C.c_int(width), be.ptr(dmap), C.c_size_t(half), be.ptr(dsrc),
                                         be.ptr(dst)), "scatter")
        want = P.scatter_model(sparse, src, np.full((n + 3, width), PAD, np.uint8))
        assert np.array_equal(rows(be, dst, width), want), n


@pytest.mark.parametrize("width", P.PERMUTE_WIDTHS)
def test_gather_scatter(be, width):
    rng = np.random.default_rng(130 + width)
    for n in P.PERMUTE_SIZES:
        nsrc = n + 37
        src = P.bit_patterns(rng, nsrc, width)
        dsrc = be.to_dev(src)
        map_out = rng.permutation(n).astype(np.uint32)
        dout = be.to_dev(map_out)
        for name, map_in in P.gather_maps(rng, n, nsrc):
            dst, din = be.filled((FRONT + n + 3) * width, np.uint8, PAD), be.to_dev(map_in)
            be.chk(be.lib.cstone_hip_gather_scatter(be.ctx, C.c_int(width), be.ptr(din),
                                                    be.ptr(dout), C.c_size_t(n), be.ptr(dsrc),
                                                    be.ptr(dst, FRONT * width)), "gather_scatter")
            got = rows(be, dst, width)
            want = P.gather_scatter_model(map_in, map_out, src, np.full((n, width), PAD, np.uint8))
            assert np.array_equal(got[FRONT:FRONT + n], want), (n, name)
            assert (got[:FRONT] == PAD).all() and (got[FRONT + n:] == PAD).all(), (n, name)


@gpu
@pytest.mark.parametrize("num_arrays", [2, 3, 4])
@pytest.mark.parametrize("width", [4, 8, 16])
def test_gather_multi(dev, width, num_arrays):
    be = dev
    rng = np.random.default_rng(140 + width)
    for n in P.PERMUTE_SIZES:
        nsrc = n + 37
        srcs = [P.bit_patterns(rng, nsrc, width) for _ in range(num_arrays)]
        dsrcs = [be.to_dev(s) for s in srcs]
        for name, map_ in P.gather_maps(rng, n, nsrc):
            dsts = [be.filled((FRONT + n + 3) * width, np.uint8, PAD) for _ in range(num_arrays)]
            dptr = (C.c_void_p * num_arrays)(*[be.ptr(d, FRONT * width).value for d in dsts])
            dmap = be.to_dev(map_)
            be.chk(be.lib.cstone_hip_gather_multi(be.ctx, C.c_int(width), be.ptr(dmap), C.c_size_t(n),
                                                  be.ptrs(dsrcs), dptr, C.c_int(num_arrays)), "gather_multi")
            for a in range(num_arrays):
                got = rows(be, dsts[a], width)
                assert np.array_equal(got[FRONT:FRONT + n], P.gather_model(map_, srcs[a])), (n, name, a)
                assert (got[:FRONT] == PAD).all() and (got[FRONT + n:] == PAD).all(), (n, name, a)
            assert n < 2 or not np.array_equal(srcs[0][map_], srcs[1][map_])  # the arrays differ


@gpu
def test_misaligned_wide_elements_are_refused(dev):
    be = dev
    map_ = be.to_dev(np.arange(4, dtype=np.uint32))
    src = be.to_dev(np.arange(8 * 64 + 16, dtype=np.uint32).view(np.uint8)[:8 * 64 + 16])
    lib = be.lib
    for width in (16, 32, 64):
        for src_off, dst_off in ((8, 0), (0, 8), (4, 4)):
            dst = be.filled(8 * 64 + 16, np.uint8, PAD)
            args = (be.ptr(src, src_off), be.ptr(dst, dst_off))
            assert lib.cstone_hip_gather(be.ctx, C.c_int(width), be.ptr(map_), C.c_size_t(4), *args) == S.E_ARG
            assert lib.cstone_hip_scatter(be.ctx, C.c_int(width), be.ptr(map_), C.c_size_t(4), *args) == S.E_ARG
            assert lib.cstone_hip_gather_scatter(be.ctx, C.c_int(width), be.ptr(map_), be.ptr(map_), C.c_size_t(4),
                                                 *args) == S.E_ARG
            assert "align" in be.last_error()
            assert (be.to_host(dst, np.uint8) == PAD).all(), (width, src_off, dst_off)


# ----------------------------------------------------------------------------------------------------------------------
# 9. argument errors
# ----------------------------------------------------------------------------------------------------------------------
@gpu
def test_unsupported_arguments_are_refused_and_empty_calls_touch_nothing(dev):
    be, lib, ctx = dev, dev.lib, dev.ctx
    n = 8
    src = be.to_dev(np.arange(64 * n, dtype=np.uint8))
    map_ = be.to_dev(np.arange(n, dtype=np.uint32))
    seg = be.to_dev(np.array([0, 4, 8], np.uint64))
    null = C.c_void_p(0)
    size = C.c_size_t
    u64, dbl = C.c_uint64, C.c_double

    def refused(call):
        """call(dst) returns CSTONE_E_ARG and leaves the device array dst as it was"""
        dst = be.filled(64 * n, np.uint8, PAD)
        assert call(be.ptr(dst)) == S.E_ARG
        assert (be.to_host(dst, np.uint8) == PAD).all()

    for bad in (0, 3, 6, 128, -4):
        refused(lambda d: lib.cstone_hip_gather(ctx, C.c_int(bad), be.ptr(map_), size(n), be.ptr(src), d))
        refused(lambda d: lib.cstone_hip_scatter(ctx, C.c_int(bad), be.ptr(map_), size(n), be.ptr(src), d))
        refused(lambda d: lib.cstone_hip_gather_scatter(ctx, C.c_int(bad), be.ptr(map_), be.ptr(map_), size(n),
                                                        be.ptr(src), d))
        refused(lambda d: lib.cstone_hip_gather_ranges(ctx, C.c_int(bad), C.c_int(32), be.ptr(seg), be.ptr(seg), C.c_int(1),
                                                       be.ptr(src), d, size(2)))
    refused(lambda d: lib.cstone_hip_gather_ranges(ctx, C.c_int(64), C.c_int(32), be.ptr(seg), be.ptr(seg), C.c_int(1),
                                                   be.ptr(src), d, size(2)))  # 64 bytes: gather yes, gather_ranges no
    refused(lambda d: lib.cstone_hip_gather_ranges(ctx, C.c_int(4), C.c_int(16), be.ptr(seg), be.ptr(seg), C.c_int(1),
                                                   be.ptr(src), d, size(2)))
    other = be.filled(64 * n, np.uint8, PAD)
    for bad_width, bad_count in ((12, 2), (2, 2), (32, 3), (4, 0), (4, 5)):
        refused(lambda d: lib.cstone_hip_gather_multi(ctx, C.c_int(bad_width), be.ptr(map_), size(n), be.ptrs([src, src]),
                                                      (C.c_void_p * 5)(d.value, *[be.ptr(other).value] * 4),
                                                      C.c_int(bad_count)))
    assert (be.to_host(other, np.uint8) == PAD).all()
    for bad in (2, 3, 16, 0):
        refused(lambda d: lib.cstone_hip_fill(ctx, C.c_int(bad), d, size(n), bytes(16)))
    for bad in (16, 0, 8):
        refused(lambda d: lib.cstone_hip_scale(ctx, C.c_int(bad), d, size(n), dbl(2.0)))
        refused(lambda d: lib.cstone_hip_increment(ctx, C.c_int(bad), be.ptr(src), d, size(n), u64(1)))
        out, res = u64(99), dbl(99.0)
        pair = (dbl * 6)(*([99.0] * 6))
        assert lib.cstone_hip_count_equal(ctx, C.c_int(bad), be.ptr(src), size(n), u64(1), C.byref(out)) == S.E_ARG
        assert lib.cstone_hip_reduce_sum(ctx, C.c_int(bad), be.ptr(src), size(n), u64(1), C.byref(out)) == S.E_ARG
        assert lib.cstone_hip_max_norm_square(ctx, C.c_int(bad), be.ptr(src), be.ptr(src), be.ptr(src), size(n),
                                              C.byref(res)) == S.E_ARG
        assert lib.cstone_hip_minmax(ctx, C.c_int(bad), be.ptr(src), size(n), pair) == S.E_ARG
        assert lib.cstone_hip_minmax_arrays(ctx, C.c_int(bad), be.ptrs([src]), C.c_int(1), size(n), pair) == S.E_ARG
        assert out.value == 99 and res.value == 99.0 and list(pair) == [99.0] * 6
    pair = (dbl * 6)(*([99.0] * 6))
    for bad_count in (0, 4):
        assert lib.cstone_hip_minmax_arrays(ctx, C.c_int(32), be.ptrs([src] * 4), C.c_int(bad_count), size(n), pair) == S.E_ARG
    assert list(pair) == [99.0] * 6
    for bad in ((32, 64, 32), (16, 32, 32), (64, 64, 16), (32, 32, 8)):
        refused(lambda d: lib.cstone_hip_segment_max(ctx, C.c_int(bad[0]), C.c_int(bad[1]), C.c_int(bad[2]), be.ptr(src),
                                                     be.ptr(seg), size(2), d))
    for bad in (5, -1, 64):
        out, value = u64(99), u64(3)
        assert lib.cstone_hip_lower_bound_value(ctx, C.c_int(bad), be.ptr(src), size(n), C.byref(value),
                                                C.byref(out)) == S.E_ARG
        assert out.value == 99
    # nothing to do: 0, with null arrays, and nothing written but a result that is defined for no elements
    assert lib.cstone_hip_gather(ctx, C.c_int(4), null, size(0), null, null) == 0
    assert lib.cstone_hip_scatter(ctx, C.c_int(4), null, size(0), null, null) == 0
    assert lib.cstone_hip_gather_scatter(ctx, C.c_int(4), null, null, size(0), null, null) == 0
    assert lib.cstone_hip_gather_multi(ctx, C.c_int(4), null, size(0), be.ptrs([None, None]), be.ptrs([None, None]),
                                       C.c_int(2)) == 0
    assert lib.cstone_hip_fill(ctx, C.c_int(4), null, size(0), bytes(8)) == 0
    assert lib.cstone_hip_scale(ctx, C.c_int(32), null, size(0), dbl(2.0)) == 0
    assert lib.cstone_hip_increment(ctx, C.c_int(32), null, null, size(0), u64(1)) == 0
    assert lib.cstone_hip_segment_max(ctx, C.c_int(32), C.c_int(32), C.c_int(32), null, null, size(0), null) == 0
    assert lib.cstone_hip_gather_ranges(ctx, C.c_int(4), C.c_int(32), null, null, C.c_int(0), null, null, size(0)) == 0
    out, res = u64(99), dbl(99.0)
    assert lib.cstone_hip_count_equal(ctx, C.c_int(32), null, size(0), u64(1), C.byref(out)) == 0 and out.value == 0
    assert lib.cstone_hip_reduce_sum(ctx, C.c_int(64), null, size(0), u64(12345), C.byref(out)) == 0 and out.value == 12345
    assert lib.cstone_hip_max_norm_square(ctx, C.c_int(64), null, null, null, size(0), C.byref(res)) == 0 and res.value == 0
    value = u64(3)
    assert lib.cstone_hip_lower_bound_value(ctx, C.c_int(1), null, size(0), C.byref(value), C.byref(out)) == 0
    assert out.value == 0
    # an empty range has no extremes: refused
    pair = (dbl * 2)(99.0, 99.0)
    assert lib.cstone_hip_minmax(ctx, C.c_int(32), be.ptr(src), size(0), pair) == S.E_ARG and list(pair) == [99.0, 99.0]
    # the context still works
    assert call_minmax(be, 32, be.to_dev(np.array([2.0, -3.0, 1.0], np.float32)), 0, 3) == [-3.0, 2.0]
