"""Inputs with a KNOWN run structure for the partial-digit sort (cstone_hip_sfc_keys_and_ordering_partial): particles
whose SFC keys, sorted on the digits from 8 * start_pass upward only, form runs of equal high bits of chosen lengths at
chosen offsets of the sorted array, with chosen low bits inside every run.  CPU only (numpy + the oracle); the GPU tests
of test_partial_sort.py check every input with `assert_structure` before they hand it to the device.

Construction: every run gets its own value of key >> shift, ascending in the order of the list; the keys are decoded to
integer cells (oracle.decode) and the particles put at the cell centres, which are exact in float and double for the
21-bit cells of 64-bit keys, in the unit box and in [-2, 2)^3 alike.  The input order is a seeded shuffle that keeps the
order of the keys of one run (so "ascending" and "descending" mean something: a run sits in input order after the
passes over the high digits), runs interleave at random."""
import os
import re

import numpy as np

from helpers import Box, end_key, key_dtype, max_level, real_dtype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PATTERNS = ("random", "third_equal", "equal", "ascending", "descending")

UNIT_BOX = Box([0, 1])
WIDE_BOX = Box([-2, 2])


def run_limit():
    """CSTONE_PARTIAL_SORT_RUN_LIMIT of the header (csrc/sort.hip ties its RUN_LIMIT to it at compile time)"""
    text = open(os.path.join(ROOT, "include", "cstone_hip.h")).read()
    return int(re.search(r"#define\s+CSTONE_PARTIAL_SORT_RUN_LIMIT\s+(\d+)", text).group(1))


def low_bits(pattern, length, shift, rng):
    """low `shift` bits of the keys of one run, in input order"""
    top = 1 << shift
    if pattern == "random":
        return rng.integers(0, top, length, dtype=np.uint64)
    if pattern == "third_equal":
        low = rng.integers(0, top, length, dtype=np.uint64)
        same = rng.permutation(length)[: max(2, length // 3)]  # at least one pair of equal keys
        low[same] = low[same[0]]
        return low
    if pattern == "equal":
        return np.full(length, rng.integers(0, top), dtype=np.uint64)
    # distinct values, sorted: `length` values out of an interval of length * step
    step = max(1, top // max(1, length))
    low = (np.arange(length, dtype=np.uint64) * np.uint64(step) + rng.integers(0, step, dtype=np.uint64))
    assert low[-1] < top and (length < 2 or (np.diff(low.astype(np.int64)) > 0).all())
    if pattern == "ascending":
        return low
    if pattern == "descending":
        return low[::-1].copy()
    raise ValueError(pattern)


def place(n, runs_at, pattern_of=None):
    """[(length, pattern)] for a sorted array of n keys in which a run of the given length starts at every given offset
    and every other key is a run of its own.  runs_at: [(offset, length)] or [(offset, length, pattern)];
    pattern_of(i) names the pattern of the i-th placed run where none is given."""
    runs, at = [], 0
    for i, item in enumerate(sorted(runs_at)):
        offset, length = item[0], item[1]
        pattern = item[2] if len(item) > 2 else (pattern_of(i) if pattern_of else PATTERNS[i % len(PATTERNS)])
        assert offset >= at, f"runs overlap at {offset}"
        runs += [(1, "random")] * (offset - at)
        runs.append((length, pattern))
        at = offset + length
    assert at <= n, f"the last run ends at {at} > n = {n}"
    runs += [(1, "random")] * (n - at)
    return runs


def offsets_of(runs):
    return np.concatenate([[0], np.cumsum([r[0] for r in runs])]).astype(np.int64)


class Case:
    """one input: positions x, y, z (real_bits), the key array to hand in (markers or zeros), what was intended"""


def build_case(oracle, curve, kb, rb, start_pass, runs, box, seed, num_markers=0, marker_stride=0):
    """runs: [(length, pattern)].  Markers are EXTRA particles (they belong to no run): marker_stride = s puts one at
    every s-th input slot (0, s, 2s, ...), otherwise num_markers of them at random slots."""
    rng = np.random.default_rng(seed)
    shift = 8 * start_pass
    levels = max_level(kb)
    num_hi = 1 << (3 * levels - shift)
    assert len(runs) <= num_hi, "more runs than values of key >> shift"
    # distinct ascending values of key >> shift, spread over the whole range
    pool = np.arange(num_hi, dtype=np.uint64) if num_hi <= (1 << 20) else \
        np.unique(rng.integers(0, num_hi, 2 * len(runs) + 16, dtype=np.uint64))
    hi = np.sort(rng.choice(pool, len(runs), replace=False))
    assert hi.size == len(runs) and (np.diff(hi.astype(np.int64)) > 0).all()
    lengths = np.array([r[0] for r in runs], dtype=np.int64)
    nv = int(lengths.sum())
    run_id = np.repeat(np.arange(len(runs)), lengths)
    low = np.concatenate([low_bits(p, l, shift, rng) for l, p in runs]) if runs else np.zeros(0, np.uint64)
    keys = (np.repeat(hi, lengths) << np.uint64(shift)) | low  # in (run, input order within the run) order
    assert (keys < end_key(kb)).all()

    # input slots: a shuffle that keeps the order inside every run
    perm = rng.permutation(nv)
    slot = perm[np.lexsort((perm, run_id))]
    keys_in = np.empty(nv, dtype=np.uint64)
    keys_in[slot] = keys

    T = real_dtype(rb)
    cells = np.array([oracle.decode(curve, kb, int(k)) for k in keys_in], dtype=np.float64).reshape(nv, 3)
    lim = box.lim
    pos = [(lim[2 * d] + (lim[2 * d + 1] - lim[2 * d]) * ((cells[:, d] + 0.5) / (1 << levels))).astype(T)
           for d in range(3)]

    # markers: extra particles at positions of their own (copies of valid ones: a lost marker shows up as a wrong key)
    if marker_stride:
        n = nv
        while n - (n + marker_stride - 1) // marker_stride < nv:
            n += 1
        assert n - (n + marker_stride - 1) // marker_stride == nv
        marked = np.zeros(n, dtype=bool)
        marked[::marker_stride] = True
    else:
        n = nv + num_markers
        marked = np.zeros(n, dtype=bool)
        marked[rng.choice(n, num_markers, replace=False)] = True
    c = Case()
    c.curve, c.kb, c.rb, c.start_pass, c.shift, c.box, c.n, c.runs = curve, kb, rb, start_pass, shift, box, n, list(runs)
    c.num_markers = int(marked.sum())
    c.x, c.y, c.z = [np.empty(n, dtype=T) for _ in range(3)]
    for dst, src in zip((c.x, c.y, c.z), pos):
        dst[~marked] = src
        dst[marked] = src[rng.integers(0, nv, c.num_markers)] if nv else T(0.25)
    c.keys_in = np.zeros(n, dtype=key_dtype(kb))
    c.keys_in[marked] = end_key(kb)
    c.intended = np.empty(n, dtype=key_dtype(kb))  # the keys the construction means the oracle to find
    c.intended[~marked] = keys_in.astype(key_dtype(kb))
    c.intended[marked] = end_key(kb)
    return c


def run_structure(keys, shift):
    """(offsets, lengths) of the runs of equal keys >> shift in the array stably sorted on those bits; markers (the end
    key) form the last run"""
    hi = np.sort(keys.astype(np.uint64) >> np.uint64(shift), kind="stable")
    if hi.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    starts = np.concatenate([[0], np.flatnonzero(hi[1:] != hi[:-1]) + 1]).astype(np.int64)
    return starts, np.diff(np.concatenate([starts, [hi.size]]))


def reference(oracle, case, honour_markers=True):
    """the oracle's keys of the input (unsorted), and its stable sort of (keys, positions)"""
    keys = oracle.compute_sfc_keys(case.curve, case.kb, case.x, case.y, case.z, case.box,
                                   case.keys_in.copy() if honour_markers else None)
    ks, order = oracle.sort_pairs(keys, np.arange(case.n))
    return keys, ks, order


def assert_structure(oracle, case):
    """the oracle finds exactly the constructed keys, and their runs have the intended lengths at the intended offsets
    (the markers behind them); returns reference(oracle, case)"""
    keys, ks, order = reference(oracle, case)
    assert np.array_equal(keys, case.intended), "the positions do not encode to the constructed keys"
    starts, lengths = run_structure(keys, case.shift)
    want_len = [r[0] for r in case.runs] + ([case.num_markers] if case.num_markers else [])
    assert lengths.tolist() == want_len, "run lengths"
    assert starts.tolist() == offsets_of(case.runs)[: len(want_len)].tolist(), "run offsets"
    # what the patterns promise, in input order: sorting on the high bits alone leaves a run in input order
    by_hi = np.argsort(keys.astype(np.uint64) >> np.uint64(case.shift), kind="stable")
    low = (keys[by_hi].astype(np.uint64) & np.uint64((1 << case.shift) - 1)).astype(np.int64)  # shift <= 48
    for (length, pattern), at in zip(case.runs, starts):
        if length < 2:
            continue
        d = np.diff(low[at: at + length])
        if pattern == "equal":
            assert (d == 0).all()
        elif pattern == "ascending":
            assert (d > 0).all()
        elif pattern == "descending":
            assert (d < 0).all()
        elif pattern == "third_equal":
            assert np.unique(low[at: at + length]).size < length
    return keys, ks, order


def intermediate_state(keys, ks, order, shift, limit):
    """what a partial sort that is NOT finished leaves: the array stably sorted on keys >> shift (every run in input
    order), with the runs of at most `limit` keys replaced by their slice of the full stable sort (ks, order).  The
    markers' run is never touched -- all its keys are equal, input order is its sorted order."""
    by_hi = np.argsort(keys.astype(np.uint64) >> np.uint64(shift), kind="stable")
    k, o = keys[by_hi].copy(), by_hi.astype(np.uint32)
    starts, lengths = run_structure(keys, shift)
    for at, length in zip(starts, lengths):
        if length <= limit:
            k[at: at + length] = ks[at: at + length]
            o[at: at + length] = order[at: at + length]
    return k, o, starts, lengths
