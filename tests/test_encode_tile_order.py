"""The order in which the re-sort's encode (csrc/sfc.hip, encodeResortKernel) walks the positions -- grid-stride, or tile by
tile so that a wave's consecutive iterations cover neighbouring positions (CSTONE_ENCODE_ORDER=stride|tile) -- changes the
order of the mover list and nothing else: a re-sorting domain under either order hands back, bit for bit, what a domain
that sorts from scratch hands back.  The sizes are those at which the tiled walk changes its path: below and at one
vector, one workgroup iteration and one tile (P = 256 VEC R positions), a partial last tile with a tail behind the last
full vector, and a grid in which some workgroups take two tiles and others one."""
import numpy as np
import pytest

from resort_support import Loop, Motion, assert_same, cloud, environment, smoothing_lengths

TILE_R = 8  # iterations per tile (2^ENCODE_TILE_LOG2 in csrc/sfc.hip)


def _run(hip, monkeypatch, kb, rb, curve, n, bucket_focus, syncs):
    from cstone_amd.domain import Domain

    rng = np.random.default_rng(11 + n % 1000)
    start = dict(pos=cloud(rng, n), h=smoothing_lengths(rng, n))  # the same cloud for the three loops
    ref = Loop(hip, kb, rb, bucket_focus, curve, n, 0, mode=Domain.SORT_FROM_SCRATCH, **start)
    loops = {order: Loop(hip, kb, rb, bucket_focus, curve, n, 0, **start) for order in ("stride", "tile")}
    motion = Motion(500 + n % 1000)
    moved = {order: 0 for order in loops}
    for step in range(syncs):
        if step:
            drawn = motion.draw(ref)
            for lp in (ref, *loops.values()):
                motion.apply(lp, drawn)
        ref.sync()
        for order, lp in loops.items():
            with environment(CSTONE_ENCODE_ORDER=order):
                lp.sync()
            assert_same(lp, ref, (n, order, step))
            st = lp.dom.stats()
            assert st["resorts"] == step, (n, order, step, st)  # one per steady sync (the first builds the tree)
            moved[order] += st["last_movers"] if step else 0
    assert ref.dom.stats()["resorts"] == 0
    return moved


@pytest.mark.gpu
@pytest.mark.parametrize("curve", [1, 0], ids=["hilbert", "morton"])
@pytest.mark.parametrize("kb,rb", [(64, 64), (32, 32)], ids=["u64-f64", "u32-f32"])
def test_tile_order_at_the_sizes_where_the_walk_changes(hip, monkeypatch, kb, rb, curve):
    vec = 16 // (rb // 8)
    P = 256 * vec * TILE_R
    sizes = [1, vec - 1, vec, 256 * vec - 1, 256 * vec, 256 * vec + 1, P - 1, P, P + 1, 3 * P + vec + 1]
    some_moved = {"stride": 0, "tile": 0}
    for n in sizes:
        moved = _run(hip, monkeypatch, kb, rb, curve, n, 8, 5)
        for order in moved:
            some_moved[order] += moved[order]
        if n >= 256 * vec:
            assert min(moved.values()) > 0, (n, moved)  # the compared path is the one under test
    assert min(some_moved.values()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("curve", [1, 0], ids=["hilbert", "morton"])
@pytest.mark.parametrize("kb,rb", [(64, 64), (32, 32)], ids=["u64-f64", "u32-f32"])
def test_tile_order_with_one_and_two_tiles_per_workgroup(hip, monkeypatch, kb, rb, curve):
    """just above 1.5 grids of tiles: half of the workgroups take two tiles, the others one, the last tile is partial and a
    tail lies behind the last full vector"""
    import torch

    vec = 16 // (rb // 8)
    P = 256 * vec * TILE_R
    grid = 4 * torch.cuda.get_device_properties(0).multi_processor_count  # (sfc.hip, computeKeysResortT)
    n = (3 * grid // 2) * P + 3
    moved = _run(hip, monkeypatch, kb, rb, curve, n, 64, 4)
    assert min(moved.values()) > 0, moved
