"""The partial-digit sort Domain::sync runs (cstone_hip_sfc_keys_and_ordering_partial: fused encode + histogram with
firstDigit > 0, radix passes from start_pass upward, fixupRunsKernel on the runs of equal high digits) on inputs whose
run structure is BUILT (partial_sort_support.py): runs of chosen lengths at chosen offsets of the sorted array -- across
the four keys of a lane, the 256 keys of a wave, the 1024 keys of a workgroup, the end of the array -- with chosen low
bits.  The reference is the oracle: compute_sfc_keys of the positions, then its stable sort_pairs of (keys, 0..n-1).
Keys, orderings, flags and extents are compared with ==."""
import numpy as np
import pytest

from oracle.oracle import HILBERT, MORTON
from helpers import Box, end_key, key_dtype, random_cloud
from partial_sort_support import (PATTERNS, UNIT_BOX, WIDE_BOX, assert_structure, build_case, intermediate_state, place,
                                  reference, run_limit, run_structure)

LIMIT = run_limit()
WAVE, GROUP = 256, 1024  # keys one wave / one workgroup of the fix-up kernel holds (4 per lane)

KEYS_PASSES = [(32, 2), (64, 2), (64, 4), (64, 6)]
combos = pytest.mark.parametrize("kb,start_pass", KEYS_PASSES)
curves = pytest.mark.parametrize("curve", [MORTON, HILBERT])
reals = pytest.mark.parametrize("rb", [32, 64])


def both_boxes(i):
    return (UNIT_BOX, WIDE_BOX)[i % 2]


# ---------------------------------------------------------------------------------------------------------------------
# the construction itself (no GPU)
# ---------------------------------------------------------------------------------------------------------------------

def test_the_run_limit_is_published_once():
    import cstone_amd

    assert LIMIT == 192 == cstone_amd.PARTIAL_SORT_RUN_LIMIT


@combos
@curves
@reals
def test_constructed_inputs_keep_their_structure(oracle, kb, start_pass, curve, rb):
    """round trip: the oracle encodes the cell centres to exactly the constructed keys, in both boxes, and the runs of
    the stably high-digit-sorted keys have the intended lengths at the intended offsets; `place` puts a run where it is
    told to; the patterns hold in input order; markers stay outside the runs"""
    runs = place(1300, [(0, 2), (3, 2), (254, 3), (510, 5), (600, LIMIT), (1000, LIMIT + 1), (1298, 2)])
    for i, box in enumerate((UNIT_BOX, WIDE_BOX)):
        case = build_case(oracle, curve, kb, rb, start_pass, runs, box, seed=kb + start_pass + i)
        keys, ks, order = assert_structure(oracle, case)
        starts, lengths = run_structure(keys, case.shift)
        found = {int(s): int(n) for s, n in zip(starts, lengths) if n > 1}
        assert found == {0: 2, 3: 2, 254: 3, 510: 5, 600: LIMIT, 1000: LIMIT + 1, 1298: 2}
        assert case.n == 1300 and np.array_equal(np.sort(order), np.arange(1300))
        # the input is shuffled: the runs do not sit together
        assert not np.array_equal(keys, ks)
    marked = build_case(oracle, curve, kb, rb, start_pass, runs, WIDE_BOX, seed=5, marker_stride=7)
    keys, ks, order = assert_structure(oracle, marked)
    assert (marked.keys_in[::7] == end_key(kb)).all() and marked.num_markers == (marked.n + 6) // 7
    assert (ks[1300:] == end_key(kb)).all() and (ks[:1300] < end_key(kb)).all()
    k, o, starts, lengths = intermediate_state(keys, ks, order, marked.shift, LIMIT)
    at = 1000  # the run past the limit stays in input order, everything else is the full sort
    assert np.array_equal(k[:at], ks[:at]) and np.array_equal(k[at + LIMIT + 1:], ks[at + LIMIT + 1:])
    assert (np.diff(o[at: at + LIMIT + 1].astype(np.int64)) > 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# on the device
# ---------------------------------------------------------------------------------------------------------------------

def dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy()).cuda()


def host(t):
    a = t.cpu().numpy()
    return a.view({np.dtype(np.int32): np.uint32, np.dtype(np.int64): np.uint64}.get(a.dtype, a.dtype))


def cbox(box):
    import cstone_amd

    return cstone_amd.make_cbox(box.lim, box.bc)


def extents_of(x, y, z):
    return tuple(float(v) for a in (x, y, z) for v in (a.min(), a.max()))


def run_partial(hip, case, finish=True, honour_markers=True, keys_in=None, unaligned=False):
    """the device call on a case; unaligned: every array handed in as a view that starts one element into a buffer"""
    keys_in = case.keys_in if keys_in is None else keys_in
    if unaligned:
        pad = lambda a: np.concatenate([a[:1], a])  # noqa: E731
        xd, yd, zd, kd = [dev(pad(a))[1:] for a in (case.x, case.y, case.z, keys_in)]
    else:
        xd, yd, zd, kd = [dev(a) for a in (case.x, case.y, case.z, keys_in)]
    keys, order, info = hip.sfc_keys_and_ordering_partial(case.curve, case.kb, xd, yd, zd, cbox(case.box),
                                                          case.start_pass, keys=kd, honour_markers=honour_markers,
                                                          finish=finish)
    hip.sync()
    return host(keys), host(order), info


def check_finished_short_runs(hip, oracle, case, unaligned=False):
    """no run passes the limit: keys and ordering are the oracle's, nothing is flagged, the extents are those of all
    inputs (None for views that do not start on a 16-byte boundary)"""
    _, ks, order = assert_structure(oracle, case)
    assert max([r[0] for r in case.runs], default=0) <= LIMIT
    for finish in (False, True):
        k, o, info = run_partial(hip, case, finish=finish, unaligned=unaligned)
        assert np.array_equal(k, ks) and np.array_equal(o, order), (finish, np.flatnonzero(k != ks)[:8])
        assert not info["run_too_long"] and not info["finished"]
        assert info["extents"] == (None if unaligned else extents_of(case.x, case.y, case.z))


@pytest.mark.gpu
@combos
@curves
@reals
def test_runs_of_two_and_three_at_lane_wave_group_and_array_edges(hip, oracle, kb, start_pass, curve, rb):
    """runs of two (swapped from registers) at sorted offsets 0, 2, 3, 255, 1023 and n - 2; runs of three (the general
    path) at 2, 254, 255, 1022 and n - 3: inside a lane's four keys, across lanes, across the wave's last lane (which
    fetches its two look-ahead keys from memory), across workgroups, at the end of the array.  n % 4 = 3, 0, 1; every
    placed run takes every low-bit pattern in turn."""
    layouts = [
        (1031, [(0, 2), (3, 2), (255, 2), (1023, 2), (1029, 2)]),
        (1032, [(2, 2), (254, 3), (1022, 3), (1029, 3)]),
        (261, [(2, 3), (255, 3), (258, 3)]),
    ]
    for li, (n, runs_at) in enumerate(layouts):
        for rot in range(len(PATTERNS)):
            runs = place(n, runs_at, lambda i: PATTERNS[(i + rot) % len(PATTERNS)])
            case = build_case(oracle, curve, kb, rb, start_pass, runs, both_boxes(li + rot), seed=100 * li + rot)
            check_finished_short_runs(hip, oracle, case)


def long_run_layout():
    """runs of 4, 5, 64, 65, LIMIT - 1 and LIMIT keys: each once inside a wave's 256 keys, once across a multiple of 256
    that is no multiple of 1024, once across a multiple of 1024"""
    L = LIMIT
    inside = [(260, 4), (270, 5), (300, 64), (520, 65), (770, L - 1), (1040, L)]
    wave = [(1278, 4), (1533, 5), (1760, 64), (2270, 65), (2500, L - 1), (2750, L)]
    group = [(2046, 4), (3070, 5), (4060, 64), (5100, 65), (6100, L - 1), (7100, L)]
    for at, n in inside:
        assert at // WAVE == (at + n - 1) // WAVE
    for at, n in wave:
        b = (at + n - 1) // WAVE * WAVE
        assert at < b <= at + n - 1 and b % GROUP != 0 and at // GROUP == (at + n - 1) // GROUP
    for at, n in group:
        assert at // GROUP + 1 == (at + n - 1) // GROUP
    return 7302, inside + wave + group


@pytest.mark.gpu
@combos
@curves
@reals
def test_runs_up_to_the_limit_inside_and_across_waves_and_workgroups(hip, oracle, kb, start_pass, curve, rb):
    """runs of 4, 5, 64, 65, 191 and 192 (the largest the fix-up takes) inside a wave's keys, across a wave boundary
    and across a workgroup boundary; every run takes every low-bit pattern in turn; n % 4 = 2"""
    n, runs_at = long_run_layout()
    for rot in range(len(PATTERNS)):
        runs = place(n, runs_at, lambda i: PATTERNS[(i + rot) % len(PATTERNS)])
        case = build_case(oracle, curve, kb, rb, start_pass, runs, both_boxes(rot), seed=7 + rot)
        check_finished_short_runs(hip, oracle, case)


@pytest.mark.gpu
@combos
@curves
@reals
def test_back_to_back_runs(hip, oracle, kb, start_pass, curve, rb):
    """a stretch of runs with no single keys between them (2, 2, 3, 2, 5, 2, 4, ...), starting at offsets 0..3 of a
    lane and reaching over several waves and a workgroup boundary: every run's first key follows another run's last"""
    lengths = [2, 2, 3, 2, 5, 2, 4, 3, 3, 2, 6, 2, 2, 7, 3, 2, 9, 2, 3, 4]
    for start in range(4):
        runs_at, at, i = [], start + 760, 0
        while at < 1400:
            runs_at.append((at, lengths[i % len(lengths)], PATTERNS[(i + start) % len(PATTERNS)]))
            at += lengths[i % len(lengths)]
            i += 1
        # ... up to the very end of the array
        case = build_case(oracle, curve, kb, rb, start_pass, place(at, runs_at), both_boxes(start), seed=start)
        check_finished_short_runs(hip, oracle, case)


@pytest.mark.gpu
@combos
@curves
@reals
def test_tiny_arrays(hip, oracle, kb, start_pass, curve, rb):
    """n = 1 .. 5 (below one lane's four keys and just above): single keys only, one run that is the whole array, and
    a run in front of or behind single keys; n = 0 succeeds with nothing flagged"""
    import torch

    import cstone_amd

    for n in (1, 2, 3, 4, 5):
        layouts = [[]] + ([[(0, n)]] if n > 1 else []) + ([[(0, n - 1)], [(1, n - 1)]] if n > 2 else [])
        for li, runs_at in enumerate(layouts):
            for rot in range(len(PATTERNS) if runs_at else 1):
                runs = place(n, runs_at, lambda i: PATTERNS[(i + rot) % len(PATTERNS)])
                case = build_case(oracle, curve, kb, rb, start_pass, runs, both_boxes(n + li + rot), seed=10 * n + rot)
                check_finished_short_runs(hip, oracle, case)
    empty = torch.zeros(0, dtype=torch.float32 if rb == 32 else torch.float64, device="cuda")
    keys, order, info = hip.sfc_keys_and_ordering_partial(curve, kb, empty, empty, empty, cbox(UNIT_BOX), start_pass)
    assert keys.numel() == 0 and order.numel() == 0
    assert info == {"run_too_long": False, "finished": False, "extents": None}
    assert cstone_amd.PARTIAL_SORT_RUN_LIMIT == LIMIT


def check_with_long_runs(hip, oracle, case):
    """some run passes the limit.  finish: flag, finishing sort, the oracle's result.  No finish: flag, and the
    intermediate state Domain::sync relies on -- runs within the limit finished, longer ones in input order."""
    keys, ks, order = assert_structure(oracle, case)
    assert max(r[0] for r in case.runs) > LIMIT
    k, o, info = run_partial(hip, case, finish=True)
    assert info["run_too_long"] and info["finished"]
    assert np.array_equal(k, ks) and np.array_equal(o, order)
    assert info["extents"] == extents_of(case.x, case.y, case.z)

    k, o, info = run_partial(hip, case, finish=False)
    assert info["run_too_long"] and not info["finished"]
    ik, io, starts, lengths = intermediate_state(keys, ks, order, case.shift, LIMIT)
    hi = k.astype(np.uint64) >> np.uint64(case.shift)
    assert (hi[1:] >= hi[:-1]).all()
    assert np.array_equal(np.sort(o), np.arange(case.n)) and np.array_equal(keys[o], k)  # a permutation of the input
    for at, length in zip(starts, lengths):
        s = slice(at, at + length)
        if length <= LIMIT or ks[at] == end_key(case.kb):
            assert np.array_equal(k[s], ks[s]) and np.array_equal(o[s], order[s]), ("finished run", at, length)
        else:
            assert (np.diff(o[s].astype(np.int64)) > 0).all(), ("run past the limit not in input order", at, length)
    assert np.array_equal(k, ik) and np.array_equal(o, io)


@pytest.mark.gpu
@combos
@curves
@reals
def test_runs_past_the_limit(hip, oracle, kb, start_pass, curve, rb):
    """runs of 193, 300 and 5000 keys with ties among short runs (a run of exactly 192 right in front of the one of
    193: the first is finished, the second is not); and 193 alone among single keys is enough to raise the flag"""
    runs_at = [(5, 2), (130, 3), (200, 300, "third_equal"), (500, 17), (600, LIMIT, "third_equal"),
               (600 + LIMIT, LIMIT + 1, "third_equal"), (1000, 64), (1100, 5000, "third_equal"), (6100, 2, "descending"),
               (6102, 3, "descending"), (6200, 100)]
    case = build_case(oracle, curve, kb, rb, start_pass, place(6311, runs_at), WIDE_BOX, seed=kb + start_pass)
    check_with_long_runs(hip, oracle, case)
    for at in (1, 250, 900):  # inside a wave, across waves, across workgroups
        case = build_case(oracle, curve, kb, rb, start_pass, place(1200, [(at, LIMIT + 1, "random")]), UNIT_BOX, seed=at)
        check_with_long_runs(hip, oracle, case)


@pytest.mark.gpu
@combos
@curves
@reals
def test_remove_markers(hip, oracle, kb, start_pass, curve, rb):
    """honour_markers: every 7th input carries the marker, or more than 192 inputs do: the markers sort last, keep
    their value and raise no flag however many they are, the runs in front of them are finished -- with the first
    marker on each of the four slots of a lane (a run reaches right up to it).  Without honour_markers a key array
    full of markers is not read at all."""
    for r in range(4):
        nv = 600 + r  # the first marker sits at sorted offset nv
        runs = place(nv, [(1, 2), (255, 3), (300, 40), (nv - 5 - r, 5 + r)])
        for markers in ({"marker_stride": 7}, {"num_markers": LIMIT + 9 + r}):
            case = build_case(oracle, curve, kb, rb, start_pass, runs, both_boxes(r), seed=r, **markers)
            assert case.n - case.num_markers == nv
            _, ks, order = assert_structure(oracle, case)
            assert (ks[nv:] == end_key(kb)).all() and (np.diff(order[nv:].astype(np.int64)) > 0).all()
            check_finished_short_runs(hip, oracle, case)
            # honour_markers = 0: the previous content of the key array, all markers here, is ignored
            ignored = np.full(case.n, end_key(kb), dtype=key_dtype(kb))
            keys0, ks0, order0 = reference(oracle, case, honour_markers=False)
            assert (ks0 < end_key(kb)).all() and run_structure(keys0, case.shift)[1].max() <= LIMIT
            k, o, info = run_partial(hip, case, keys_in=ignored, honour_markers=False)
            assert np.array_equal(k, ks0) and np.array_equal(o, order0)
            assert not info["run_too_long"] and not info["finished"]
    # markers next to a run past the limit: the flag is the run's, the markers stay where they are
    runs = place(700, [(3, 2), (700 - LIMIT - 1, LIMIT + 1, "third_equal")])
    case = build_case(oracle, curve, kb, rb, start_pass, runs, WIDE_BOX, seed=9, num_markers=LIMIT + 30)
    check_with_long_runs(hip, oracle, case)


@pytest.mark.gpu
@combos
@curves
@reals
def test_unaligned_views(hip, oracle, kb, start_pass, curve, rb):
    """x[1:], y[1:], z[1:], keys[1:]: the plain encode and the sort's own histogram with start_pass > 0; the same
    results, extents reported as not measured"""
    n, runs_at = long_run_layout()
    case = build_case(oracle, curve, kb, rb, start_pass, place(n, runs_at), WIDE_BOX, seed=3, marker_stride=7)
    check_finished_short_runs(hip, oracle, case, unaligned=True)
    runs = place(1203, [(0, 2), (250, LIMIT + 1, "third_equal"), (1200, 3)])
    case = build_case(oracle, curve, kb, rb, start_pass, runs, UNIT_BOX, seed=4)
    keys, ks, order = assert_structure(oracle, case)
    k, o, info = run_partial(hip, case, finish=True, unaligned=True)
    assert info == {"run_too_long": True, "finished": True, "extents": None}
    assert np.array_equal(k, ks) and np.array_equal(o, order)
    k, o, info = run_partial(hip, case, finish=False, unaligned=True, honour_markers=False)
    ik, io, _, _ = intermediate_state(keys, ks, order, case.shift, LIMIT)
    assert info == {"run_too_long": True, "finished": False, "extents": None}
    assert np.array_equal(k, ik) and np.array_equal(o, io)


@pytest.mark.gpu
@pytest.mark.parametrize("kb", [32, 64])
@curves
@reals
def test_extents_are_those_of_all_inputs(hip, oracle, kb, curve, rb):
    """aligned arrays: the fused kernel's extents equal numpy's min / max over all n inputs, removal-flagged ones
    included, for n below one 16-byte vector, n = k VEC + r and a box that does not start at 0"""
    box = Box([-1.5, 2.5, 3.0, 4.0, -8.0, -6.0])
    vec = 16 // (rb // 8)
    for n in sorted({1, vec - 1, vec, vec + 1, 5 * vec + 1, 1000 * vec + vec - 1, 70001}):
        x, y, z = random_cloud(n, box, rb, seed=n)
        keys_in = np.zeros(n, dtype=key_dtype(kb))
        keys_in[::3] = end_key(kb)
        # the extreme particles are flagged for removal: they count all the same
        for a in (x, y, z):
            keys_in[[a.argmin(), a.argmax()]] = end_key(kb)
        ref = oracle.compute_sfc_keys(curve, kb, x, y, z, box, keys_in.copy())
        ks, order = oracle.sort_pairs(ref, np.arange(n))
        keys, o, info = hip.sfc_keys_and_ordering_partial(curve, kb, dev(x), dev(y), dev(z), cbox(box), 0,
                                                          keys=dev(keys_in))
        hip.sync()
        assert info["extents"] == extents_of(x, y, z), n
        assert not info["run_too_long"] and not info["finished"]
        assert np.array_equal(host(keys), ks) and np.array_equal(host(o), order)


@pytest.mark.gpu
@pytest.mark.parametrize("kb,rb", [(32, 32), (32, 64), (64, 32), (64, 64)])
@curves
def test_start_pass_zero_equals_the_full_entry(hip, kb, rb, curve):
    """start_pass = 0: byte-equal keys and ordering to cstone_hip_sfc_keys_and_ordering, markers included"""
    import torch

    box = Box([-1.0, 2.0, 0.0, 1.0, 3.0, 7.0])
    for n, off in ((1, 0), (5003, 0), (5003, 1), (70001, 0)):
        x, y, z = random_cloud(n + off, box, rb, seed=n + kb, kind="clustered")
        xd, yd, zd = [dev(a)[off:] for a in (x, y, z)]
        marked = torch.zeros(n, dtype=torch.int64 if kb == 64 else torch.int32, device="cuda")
        marked[::5] = -(1 << 63) if kb == 64 else 1 << 30
        k1, v1 = hip.sfc_keys_and_ordering(curve, kb, xd, yd, zd, cbox(box), keys=marked.clone())
        k2, v2, info = hip.sfc_keys_and_ordering_partial(curve, kb, xd, yd, zd, cbox(box), 0, keys=marked.clone())
        hip.sync()
        assert torch.equal(k1, k2) and torch.equal(v1, v2)
        assert not info["run_too_long"] and not info["finished"] and (info["extents"] is None) == (off == 1)


# ---- both tile shapes of the radix passes, input that is not constructed

N_LARGE = (1 << 20) + 4099
LARGE_BOX = Box([-1.0, 3.0, 2.0, 4.0, -5.0, 1.0])
_clouds = {}


def large_cloud(oracle, collapsed):
    """uniform positions in a non-unit box (or the same cloud scaled into a cube of 1e-6), the oracle's keys and sort:
    computed once, shared, never changed"""
    if collapsed not in _clouds:
        x, y, z = random_cloud(N_LARGE, LARGE_BOX, 64, seed=11)
        if collapsed:
            x, y, z = [c + (a - a.min()) / (a.max() - a.min()) * 1e-6 for a, c in zip((x, y, z), (0.7, 2.9, -1.1))]
        keys = oracle.compute_sfc_keys(HILBERT, 64, x, y, z, LARGE_BOX)
        ks, order = oracle.sort_pairs(keys, np.arange(N_LARGE))
        for a in (x, y, z, keys, ks, order):
            a.setflags(write=False)
        _clouds[collapsed] = (x, y, z, keys, ks, order)
    return _clouds[collapsed]


@pytest.mark.gpu
@pytest.mark.parametrize("start_pass", [2, 4, 6])
@pytest.mark.parametrize("collapsed", [False, True])
def test_more_than_a_million_particles(hip, oracle, start_pass, collapsed):
    """n = 2^20 + 4099 takes the 16 Ki-pair tiles.  Uniform: no run passes the limit (asserted on the oracle's keys),
    nothing is flagged.  Collapsed into 1e-6: runs far past it, the finishing sort gives the oracle's result."""
    x, y, z, keys, ks, order = large_cloud(oracle, collapsed)
    longest = int(run_structure(keys, 8 * start_pass)[1].max())
    assert longest > LIMIT if collapsed else longest <= LIMIT, longest
    k, o, info = hip.sfc_keys_and_ordering_partial(HILBERT, 64, dev(x), dev(y), dev(z), cbox(LARGE_BOX), start_pass)
    hip.sync()
    assert info["run_too_long"] == collapsed and info["finished"] == collapsed
    assert info["extents"] == extents_of(x, y, z)
    assert np.array_equal(host(k), ks) and np.array_equal(host(o), order)


@pytest.mark.gpu
def test_32_bit_keys_of_300000_uniform_particles(hip, oracle):
    """key_bits 32 / start_pass 2 on input that is not constructed: whether the fix-up suffices is what the oracle's
    keys say (14 high bits for 300000 particles: about 18 per run)"""
    n = 300000
    x, y, z = random_cloud(n, LARGE_BOX, 32, seed=12)
    keys = oracle.compute_sfc_keys(MORTON, 32, x, y, z, LARGE_BOX)
    ks, order = oracle.sort_pairs(keys, np.arange(n))
    too_long = bool(run_structure(keys, 16)[1].max() > LIMIT)
    assert not too_long  # uniform: no run comes near the limit
    k, o, info = hip.sfc_keys_and_ordering_partial(MORTON, 32, dev(x), dev(y), dev(z), cbox(LARGE_BOX), 2)
    hip.sync()
    assert info["run_too_long"] == too_long and info["finished"] == too_long
    assert np.array_equal(host(k), ks) and np.array_equal(host(o), order)


@pytest.mark.gpu
@pytest.mark.parametrize("kb", [32, 64])
def test_argument_errors(hip, kb):
    """an odd start_pass is refused, not rounded; so are start_pass = key_bits / 8 and a negative one (CSTONE_E_ARG);
    a workspace that is too small is CSTONE_E_CAPACITY"""
    import torch

    import cstone_amd

    n = 1000
    x, y, z = [dev(a) for a in random_cloud(n, UNIT_BOX, 64, seed=1)]
    for bad in (1, 3, kb // 8 - 1, kb // 8, kb // 8 + 2, -1, -2):
        with pytest.raises(cstone_amd.CstoneError, match=r"failed \(-1\)"):
            hip.sfc_keys_and_ordering_partial(HILBERT, kb, x, y, z, cbox(UNIT_BOX), bad)
    small = torch.empty(hip.sort_temp_bytes(kb, n) - 256, dtype=torch.uint8, device="cuda")
    with pytest.raises(cstone_amd.CstoneError, match=r"failed \(-2\)"):
        hip.sfc_keys_and_ordering_partial(HILBERT, kb, x, y, z, cbox(UNIT_BOX), 2, temp=small)
    # ... and the largest legal start_pass is fine
    _, _, info = hip.sfc_keys_and_ordering_partial(HILBERT, kb, x, y, z, cbox(UNIT_BOX), kb // 8 - 2)
    hip.sync()
    assert not info["finished"] or info["run_too_long"]
