"""TEST INFRASTRUCTURE for tests/test_primitives.py: where the streaming kernels of csrc/primitives.hip and
csrc/extras.hip change their path (the sizes and the positions inside an array that each loop of a kernel reads), the
builders of the inputs, and the numpy models of the entry points.

Models.  Each one restates the CONTRACT of its entry -- the comment in include/cstone_hip.h -- in plain numpy or Python
integers; none follows a kernel.  The geometry functions (minmax_*, norm_*) do follow the kernels' launch rules: they say
WHERE to plant a value so that a given loop is the one that has to find it, never what the result is.  The unmarked
tests of test_primitives.py check every builder against its own premise before a GPU sees its output."""
import numpy as np

EDGE_SIZES = (1, 255, 256, 257, 1023, 1024, 1025)
PERMUTE_WIDTHS = (1, 2, 4, 8, 12, 16, 24, 32, 64)   # gather / scatter / gather_scatter
RANGE_WIDTHS = (1, 2, 4, 8, 12, 16, 24, 32)         # gather_ranges
CU_COUNTS = (64, 256, 304)                          # the parts the geometry is checked for without a GPU
M64 = (1 << 64) - 1


def real(bits):
    return {32: np.float32, 64: np.float64}[bits]


def uint(bits):
    return {32: np.uint32, 64: np.uint64}[bits]


def noise(rng, n, dtype, scale=1.0):
    """seeded noise strictly inside (-scale, scale), also after rounding to dtype"""
    a = rng.uniform(-1.0, 1.0, n).astype(dtype)
    one = dtype(1.0)
    return np.clip(a, np.nextafter(-one, dtype(0)), np.nextafter(one, dtype(0))) * dtype(scale)


def bit_patterns(rng, n, width):
    """n elements of `width` arbitrary bytes each, as an (n, width) uint8 array; from 4 bytes on no two rows are equal (the first four bytes
    count the rows)"""
    a = rng.integers(0, 256, (n, width), dtype=np.uint8)
    if width >= 4:
        a[:, :4] = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4) ^ a[:1, :4]
    return a


# ----------------------------------------------------------------------------------------------------------------------
# minmax: grid = min(8 numCu, ceil(n / 256)) workgroups of 256 lanes read packs of 16 bytes behind a scalar head (up to
# the first 16-byte boundary); a lane steps by stride = 256 grid packs, four packs per step while that many are left
# ----------------------------------------------------------------------------------------------------------------------
HEAD, FOUR, SINGLE, TAIL = 0, 1, 2, 3


def minmax_sizes(itemsize, num_cu):
    """one_trip: the issue's `one more than VEC 8 256 numCu` (every lane reads exactly one pack, one scalar behind them);
    second_trip: two packs more, so that lane 0 takes a second step of the single loop at any alignment; four_deep: lanes 0..1023 take one
    four-deep step, the others three single ones, and a scalar tail is left"""
    vec = 16 // itemsize
    s = 8 * 256 * num_cu
    return {"one_trip": vec * s + 1, "second_trip": vec * (s + 2) + 1, "four_deep": vec * 3 * s + 4 * vec * 256 + 3}


def minmax_layout(n, offset, itemsize, num_cu):
    """(head, packs, vec, stride) for an array that starts `offset` elements behind a 16-byte boundary"""
    vec = 16 // itemsize
    head = min((vec - offset % vec) % vec, n)
    return head, (n - head) // vec, vec, min(8 * num_cu, -(-n // 256)) * 256


def minmax_reader(n, offset, itemsize, num_cu):
    """for every element: which part of the kernel reads it (HEAD, FOUR, SINGLE, TAIL) and in which trip of that loop"""
    head, npk, vec, stride = minmax_layout(n, offset, itemsize, num_cu)
    p = np.arange(npk, dtype=np.int64)
    lane, step = p % stride, p // stride
    deep = np.where(lane + 3 * stride < npk, (npk - 3 * stride - lane - 1) // (4 * stride) + 1, 0)
    four = step < 4 * deep
    tail = n - head - npk * vec
    part = np.concatenate([np.full(head, HEAD), np.repeat(np.where(four, FOUR, SINGLE), vec), np.full(tail, TAIL)])
    trip = np.concatenate([np.zeros(head, np.int64), np.repeat(np.where(four, step // 4, step - 4 * deep), vec),
                           np.zeros(tail, np.int64)])
    return part, trip


def minmax_plants(n, offset, itemsize, num_cu):
    """name -> index of the places where an extreme is planted; a name is present only where the array has that place"""
    head, npk, vec, stride = minmax_layout(n, offset, itemsize, num_cu)
    p = {"first": 0, "last": n - 1}
    if head > 1:
        p["head_last"] = head - 1
    if head + npk * vec < n - 1:
        p["tail_first"] = head + npk * vec
    deep_lanes = npk - 3 * stride  # the lanes whose first step is four packs deep
    if deep_lanes > 0:
        assert deep_lanes <= stride  # one four-deep step at the most: what the closed forms below assume
        p["four_first"] = head
        p["four_last_load_first"] = head + 3 * stride * vec
        p["four_last"] = head + npk * vec - 1
        if deep_lanes < stride:
            p["single_first"] = head + deep_lanes * vec
            p["single_last"] = head + 3 * stride * vec - 1
    elif npk > stride:
        p["trip1_last"] = head + stride * vec - 1
        p["trip2_first"] = head + stride * vec
    return p


def extremes_with(view, lo, hi, planted):
    """{min, max} of `view` (whose own are lo, hi) with the elements at planted = {index: value} replaced"""
    vals = list(planted.values())
    if view.size == len(planted):
        return [float(min(vals)), float(max(vals))]
    if any(view[i] == lo or view[i] == hi for i in planted):
        keep = np.ones(view.size, bool)
        keep[list(planted)] = False
        lo, hi = view[keep].min(), view[keep].max()
    return [float(min([lo] + vals)), float(max([hi] + vals))]


# ----------------------------------------------------------------------------------------------------------------------
# grid-stride reductions: count_equal / reduce_sum on min(8 numCu, ceil(n / 256)) workgroups, max_norm_square on
# min(4 numCu, ceil(n / 256))
# ----------------------------------------------------------------------------------------------------------------------
def count_big(num_cu):
    return 2 * 8 * 256 * num_cu + 77


def norm_big(num_cu):
    return 2 * 4 * 256 * num_cu + 5


def stride_of(n, per_cu, num_cu):
    return min(per_cu * num_cu, -(-n // 256)) * 256


def norm_plants(n, num_cu):
    """name -> index: the last element, the second and third stride, each wave of the last workgroup (first trip)"""
    s = stride_of(n, 4, num_cu)
    p = {"last": n - 1}
    if s + 5 < n:
        p["stride2"] = s + 5
    if 2 * s + 2 < n:
        p["stride3"] = 2 * s + 2
    for w in range(4):
        i = s - 256 + 64 * w + 13
        if i < n:
            p[f"last_group_wave{w}"] = i
    return p


def exact_sum(a):
    """sum of an unsigned array as a Python integer (no wrap): the two 32-bit halves summed apart"""
    a = np.asarray(a).astype(np.uint64)
    return (int((a >> np.uint64(32)).sum(dtype=np.uint64)) << 32) + int((a & np.uint64(0xFFFFFFFF)).sum(dtype=np.uint64))


def sum_cases(rng, bits, n):
    """[(name, data, init)] for reduce_sum.  u32: values just below 2^32, so two elements pass 2^32 and a million reach
    2^52; u64: values above 2^63, so two elements wrap 2^64; a single element wraps through init"""
    dt = uint(bits)
    top = 1 << bits
    data = rng.integers(top - (1 << 20), top, n, dtype=np.uint64, endpoint=False).astype(dt) if bits == 32 else \
        rng.integers(1 << 63, M64, n, dtype=np.uint64)
    last = np.zeros(n, dt)
    last[-1] = top - 3
    return [("near_top", data, 5), ("only_last", last, 0), ("init_near_2^63", data, (1 << 63) - 2),
            ("init_wraps", data, M64 - 2)]


def reduce_sum_model(data, init):
    """cstone_hip.h, reduce_sum: init + sum of the elements in 64-bit arithmetic"""
    return (init + exact_sum(data)) & M64


def count_cases(rng, bits, n, num_cu):
    """[(name, data, value)] for count_equal"""
    dt = uint(bits)
    s = stride_of(n, 8, num_cu)
    value = 0xFFFFFFF0 if bits == 32 else (0xABCD0123 << 32) | 0x89ABCDEF
    other = rng.integers(0, 50, n).astype(dt)
    out = []
    a = other.copy()
    a[-1] = value
    out.append(("last_only", a, value))
    if s + 11 < n:
        a = other.copy()
        a[[s, s + 11, n - 2]] = value
        out.append(("second_stride_only", a, value))
    out.append(("nowhere", other.copy(), value))
    out.append(("everywhere", np.full(n, value, dt), value))
    out.append(("many", other.copy(), 7))
    if bits == 64:
        # the low word matches in two elements of three, the whole value in every 97th
        a = rng.integers(1, 1 << 31, n).astype(np.uint64) << np.uint64(32)
        a[::3] = 0
        a |= np.where(np.arange(n) % 3 != 2, np.uint64(value & 0xFFFFFFFF), np.uint64(5))
        a[::97] = value
        out.append(("low_word_matches", a, value))
    return out


def increment_cases(rng, bits, n):
    """[(name, data, value)] for increment: wrap at 2^bits; for 32 bits a value above 2^32, whose low word is added"""
    dt = uint(bits)
    top = 1 << bits
    near = (top - 1 - rng.integers(0, 100, n)).astype(np.uint64).astype(dt) if bits == 32 else \
        np.uint64(M64) - rng.integers(0, 100, n).astype(np.uint64)
    near[::2] = rng.integers(0, 1000, near[::2].size).astype(dt)
    out = [("wraps", near, 1000), ("top_bit", near, (top >> 1) + 5)]
    if bits == 32:
        out.append(("value_above_2^32", near, (5 << 32) | 17))
    return out


def increment_model(data, value):
    """cstone_hip.h, increment: out[i] = in[i] + value in the elements' own unsigned arithmetic"""
    mask = (1 << (data.dtype.itemsize * 8)) - 1
    return ((data.astype(np.uint64) + np.uint64(value & mask)) & np.uint64(mask)).astype(data.dtype)


def norm_model(x, y, z):
    """cstone_hip.h, max_norm_square: max of x^2 + y^2 + z^2 evaluated in the arrays' own precision, left to right and
    without fused multiply-adds; 0 for no elements"""
    return float(((x * x + y * y) + z * z).max()) if x.size else 0.0


# ----------------------------------------------------------------------------------------------------------------------
# segment_max
# ----------------------------------------------------------------------------------------------------------------------
SEGMENT_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 1000)
SEGMENT_COUNTS = (15, 16, 17, 255, 256, 257)


def segment_length_lists(rng):
    """[(name, lengths)]: every listed length first and last of a call (the nine rotations of the list, a run of empty
    segments in the middle of each), the counts around 16 and 256, a list for the lane positions and 5000 random ones"""
    base = list(SEGMENT_LENGTHS)
    out = []
    for r in range(len(base)):
        rot = base[r:] + base[:r]
        out.append((f"rotation{r}", rot[:4] + [0, 0, 0] + rot[4:]))
    for ns in SEGMENT_COUNTS:
        out.append((f"count{ns}", [base[(i + ns) % len(base)] for i in range(ns)]))
    out.append(("lanes", [33] * 17 + [17] * 17))
    rand = rng.integers(0, 90, 5000)
    rand[100:104] = 0
    rand[-2:] = 0
    out.append(("random5000", [int(v) for v in rand]))
    return out


def segment_offsets(lengths, index_bits, start=5):
    return (start + np.concatenate([[0], np.cumsum(lengths)])).astype(uint(index_bits))


def segment_values(rng, lengths, kind, in_bits, start=5, guard=3):
    """values for the segments (which begin at element `start`); in front of them and behind them lie `start` resp.
    `guard` elements larger than any other, which belong to no segment.
    positive: noise in (0, 1) and the maximum of segment s, above 1, at position s % 17 (or the last one of a shorter
    segment); negative: all in (-1, 0); mixed: noise in (-1, 1), every third segment wholly negative.
    Returns (values, position of the planted maximum in each segment, -1 where none)."""
    dt = real(in_bits)
    total = int(np.sum(lengths))
    u = np.abs(noise(rng, total, np.float64))
    u[u == 0] = 0.5
    if kind == "positive":
        v = u
    elif kind == "negative":
        v = -u
    else:
        v = noise(rng, total, np.float64)
    at = np.full(len(lengths), -1)
    a = 0
    for s, ln in enumerate(lengths):
        if kind == "positive" and ln:
            at[s] = min(s % 17, ln - 1)
            v[a + at[s]] = 1.0 + (s % 7 + 1) * np.pi / 30  # not representable in float
        if kind == "mixed" and s % 3 == 0:
            v[a:a + ln] = -np.abs(v[a:a + ln]) - 1e-3
        a += ln
    full = np.concatenate([np.full(start, 1e9), v, np.full(guard, 1e9)])
    return full.astype(dt), at


def segment_max_model(values, offsets, out_bits):
    """cstone_hip.h, segment_max: out[s] = max(0, in[segments[s] .. segments[s+1])) in the precision of `in`, then
    converted to the output type; an empty segment gives 0"""
    out = np.zeros(offsets.size - 1, real(out_bits))
    for s in range(out.size):
        a, b = int(offsets[s]), int(offsets[s + 1])
        m = values.dtype.type(0)
        if b > a:
            m = max(m, values[a:b].max())
        out[s] = real(out_bits)(m)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# gather_ranges
# ----------------------------------------------------------------------------------------------------------------------
def range_cases(rng, buffer_size, nsrc, index_bits):
    """[(name, scan[num_ranges + 1], offsets[num_ranges])].  `ranges`: up to seven non-empty ranges with two empty ones
    in front, three in a row in the middle and two at the end; the source interval of the second non-empty range touches
    that of the first, the third overlaps the second; the others lie anywhere (with 64-bit indices: above 2^16).
    `single`: one range."""
    dt = uint(index_bits)
    floor = (1 << 16) + 1 if index_bits == 64 else 0
    k = min(buffer_size, 7)
    cuts = np.sort(rng.choice(np.arange(1, buffer_size), k - 1, replace=False)) if k > 1 else np.zeros(0, np.int64)
    full = [int(v) for v in np.diff(np.concatenate([[0], cuts, [buffer_size]]))]
    lengths = [0, 0] + full[:k // 2] + [0, 0, 0] + full[k // 2:] + [0, 0]
    offsets, prev = [], None
    seen = 0
    for ln in lengths:
        o = int(rng.integers(floor, nsrc - ln + 1))
        if ln:
            if seen == 0:
                o = int(rng.integers(floor, nsrc - sum(full[:3]) + 1))  # room for the two that follow it
            elif seen == 1:
                o = prev[0] + prev[1]            # touches
            elif seen == 2:
                o = prev[0] + prev[1] // 2       # overlaps (or touches, if the range before holds one element)
            seen += 1
            prev = (o, ln)
        offsets.append(o)
    assert max(o + ln for o, ln in zip(offsets, lengths)) <= nsrc
    scan = np.concatenate([[0], np.cumsum(lengths)]).astype(dt)
    single_off = int(rng.integers(floor, nsrc - buffer_size + 1))
    return [("ranges", scan, np.array(offsets, dt)), ("single", np.array([0, buffer_size], dt), np.array([single_off], dt))]


def gather_ranges_model(scan, offsets, src):
    """cstone_hip.h, gather_ranges: buffer[i] = src[range_offsets[r] + i - range_scan[r]] for the range r with
    range_scan[r] <= i < range_scan[r+1]"""
    parts = [src[int(o):int(o) + int(b) - int(a)] for a, b, o in zip(scan[:-1], scan[1:], offsets)]
    return np.concatenate(parts) if parts else src[:0]


# ----------------------------------------------------------------------------------------------------------------------
# lower_bound_value
# ----------------------------------------------------------------------------------------------------------------------
LOWER_BOUND_KINDS = {0: np.uint32, 1: np.uint64, 2: np.int32, 3: np.int64, 4: np.float32}
LOWER_BOUND_SIZES = (1, 2, 255, 5000)


def lower_bound_cases(rng, kind, n):
    """[(sorted array, [(name, value)])] of dtype LOWER_BOUND_KINDS[kind].  Integers span the whole type but its two end
    values (so u32 reaches above 2^31, u64 above 2^63, the signed ones below 0), with runs of equal elements and gaps;
    floats: one finite array with subnormals of both signs, one with -inf and +inf as elements."""
    dt = LOWER_BOUND_KINDS[kind]
    if kind == 4:
        tiny = np.float32(1e-42)  # subnormal
        pool = np.concatenate([noise(rng, n, np.float32, 1e30), noise(rng, n, np.float32, 1e-3),
                               noise(rng, n, np.float32, 1.0) * tiny]).astype(np.float32)
        pool = pool[pool != 0]
        a = np.sort(rng.choice(pool, n, replace=False)) if n > 2 else np.sort(np.array([-tiny, tiny * 3][:n], np.float32))
        if n > 4:
            a[n // 3:n // 3 + 3] = a[n // 3]  # a run of equal elements
            a = np.sort(a)
        arrays = [a]
        if n >= 2:
            b = a.copy()
            b[0], b[-1] = -np.inf, np.inf
            if n > 4:
                b[1], b[-2] = -np.inf, np.inf  # runs of infinities
            arrays.append(b)
        below, above = [np.float32(-np.inf)], [np.float32(np.inf)]
    else:
        info = np.iinfo(dt)
        lo, hi = int(info.min) + 2, int(info.max) - 2
        span = hi - lo
        picks = sorted(lo + ((int(rng.integers(0, 1 << 62)) << 2) | int(rng.integers(0, 4))) % span for _ in range(n))
        a = np.array(picks, dtype=object)
        if n > 4:
            a[n // 3:n // 3 + 4] = a[n // 3]          # a run of equal elements
            a[-3:] = a[-1]                            # and one at the end
            a = np.array(sorted(a), dtype=object)
        arrays = [np.array([int(v) for v in a], dtype=dt)]
        below, above = [dt(info.min), dt(int(arrays[0][0]) - 1)], [dt(info.max), dt(int(arrays[0][-1]) + 1)]
    out = []
    for a in arrays:
        uniq, first, counts = np.unique(a, return_index=True, return_counts=True)
        values = [("below", v) for v in below] + [("above", v) for v in above]
        once = uniq[counts == 1]
        runs = uniq[counts > 1]
        values += [("present_once", v) for v in (once[:1].tolist() + once[once.size // 2:once.size // 2 + 1].tolist() +
                                                  once[-1:].tolist())]
        values += [("first_of_run", v) for v in runs[:3].tolist() + runs[-1:].tolist()]
        if a.size >= 2 and kind != 4:
            for i in sorted({0, (a.size - 1) // 2, a.size - 2}):
                if int(a[i + 1]) - int(a[i]) >= 2:
                    values.append(("absent", int(a[i]) + 1))
        if a.size >= 2 and kind == 4:
            for i in sorted({0, (a.size - 1) // 2, a.size - 2}):
                if not (np.isfinite(a[i]) and np.isfinite(a[i + 1])):
                    continue
                mid = np.float32((np.float64(a[i]) + np.float64(a[i + 1])) / 2)
                if a[i] < mid < a[i + 1]:
                    values.append(("absent", mid))
            values += [("subnormal", np.float32(1e-42)), ("subnormal", np.float32(-1e-42))]
        out.append((a, [(name, dt(v)) for name, v in values]))
    return out


def lower_bound_model(a, value):
    """cstone_hip.h, lower_bound_value: index of the first element >= value in the order of the element type"""
    return int(np.searchsorted(a, a.dtype.type(value), side="left"))


# ----------------------------------------------------------------------------------------------------------------------
# gather / scatter / gather_scatter / gather_multi / fill on elements of `width` bytes: (n, width) uint8 arrays
# ----------------------------------------------------------------------------------------------------------------------
PERMUTE_SIZES = EDGE_SIZES + (4097,)


def gather_maps(rng, n, nsrc):
    """[(name, map)]: random indices with repeats (first and last source element among them), all indices equal"""
    m = rng.integers(0, nsrc, n).astype(np.uint32)
    m[0] = nsrc - 1
    m[-1] = 0 if n > 1 else m[-1]
    if n > 2:
        m[n // 2] = m[n // 2 - 1]
    return [("repeats", m), ("all_equal", np.full(n, min(nsrc - 1, 3), np.uint32))]


def gather_model(map_, src):
    """cstone_hip.h, gather: dst[i] = src[map[i]]"""
    return src[map_]


def scatter_model(map_, src, dst):
    """cstone_hip.h, scatter: dst[map[i]] = src[i]; the other elements of dst stay"""
    out = dst.copy()
    out[map_] = src[:map_.size]
    return out


def gather_scatter_model(map_in, map_out, src, dst):
    """cstone_hip.h, gather_scatter: dst[map_out[i]] = src[map_in[i]]"""
    out = dst.copy()
    out[map_out] = src[map_in]
    return out
