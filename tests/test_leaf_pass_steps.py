"""The step plan of the leaf pass (csrc/leaf_steps.hpp, leafSortWaveKernel in csrc/resort.hip) at the smallest shapes at
which it can go wrong: fewer leaves than waves, tiles whose last quarter is empty or partial, every number of leaves per
tile, and the step kinds side by side inside one quarter (four leaves per step next to two, leaves of 64 / 65 and 128 / 129
slots as the first and as the second leaf of a step, empty leaves).  A domain that re-sorts and one that always sorts from
scratch step side by side, as in test_resort.py, and everything they return is compared bit for bit; each case runs with
either flavour of the kernel forced (CSTONE_RESORT_PAIRS)."""
import numpy as np
import pytest


class _Stepper:
    """a client's time-stepping loop: the arrays a sync returns are moved in place and handed to the next sync"""

    def __init__(self, hip, kb, bucket_focus, curve, pos, seed, allow_resort):
        import torch

        import cstone_amd
        from cstone_amd.domain import Domain

        rng = np.random.default_rng(seed)
        n = pos.shape[0]
        self.hip, self.allow = hip, allow_resort
        kdt = torch.int64 if kb == 64 else torch.int32
        # periodic: the box is [0, 1) whatever the particles do, so no move re-encodes every key
        box = cstone_amd.make_cbox([0, 1, 0, 1, 0, 1], (1, 1, 1))
        self.dom = Domain(hip, curve, kb, 64, max(bucket_focus, 64) * 4, bucket_focus, 0.5, box)
        self.x, self.y, self.z = [torch.from_numpy(np.ascontiguousarray(pos[:, d])).cuda() for d in range(3)]
        self.h = torch.from_numpy(rng.uniform(0.001, 0.01, n)).cuda()
        self.ident = torch.arange(n, dtype=torch.float64, device="cuda")  # follows its particle through every sync
        self.keys = torch.zeros(n, dtype=kdt, device="cuda")
        self.scratch = torch.empty_like(self.x)

    def sync(self):
        self.dom.set_sort_mode(self.dom.SORT_INCREMENTAL if self.allow else self.dom.SORT_FROM_SCRATCH)
        self.keys, self.x, self.y, self.z, self.h, self.scratch, (self.ident,) = self.dom.sync(
            self.keys, self.x, self.y, self.z, self.h, self.scratch, [self.ident])
        self.hip.sync()
        return dict(keys=self.keys.cpu().numpy(), x=self.x.cpu().numpy(), y=self.y.cpu().numpy(),
                    z=self.z.cpu().numpy(), h=self.h.cpu().numpy(), ident=self.ident.cpu().numpy(), view=self.dom.view())

    def move(self, kind, mrng):
        """in place, on the arrays the last sync returned"""
        import torch

        coords = (self.x, self.y, self.z)
        m = self.x.numel()

        def put(sel, values, a):
            a[sel] = torch.from_numpy(values).to(a.dtype).cuda()

        def chosen(count):
            return torch.from_numpy(mrng.choice(m, max(1, count), replace=False)).cuda()

        if kind == "none":
            return
        if kind in ("jitter", "drift"):  # everybody, by a fraction of a leaf: few change their leaf, or many
            for a in coords:
                a.add_(torch.from_numpy(mrng.normal(0, 2e-4 if kind == "jitter" else 2e-3, m)).cuda()).clamp_(0.0, 1.0 - 1e-9)
        elif kind in ("few", "many"):  # 2 % (or every second particle) jump anywhere: leaves drain and fill
            sel = chosen(m // (50 if kind == "few" else 2))
            for a in coords:
                put(sel, mrng.uniform(0, 1 - 1e-9, sel.numel()), a)
        elif kind in ("collapse", "gather"):
            # a tenth of the particles onto three points (overfull leaves), or 2 % onto forty points next to particles that
            # stay: a dozen arrivals per point and a small offset each, so leaves of up to 64 slots grow past 64 and some
            # past 128 without reaching the limit of the leaf pass
            sel = chosen(m // 10 if kind == "collapse" else m // 50)
            if kind == "collapse":
                pts, spread = mrng.uniform(0.1, 0.9, (3, 3)), 0.0
            else:
                at = torch.from_numpy(mrng.choice(m, 40, replace=False)).cuda()
                pts, spread = np.stack([a[at].cpu().numpy() for a in coords], axis=1), 1e-7
            which = mrng.integers(0, pts.shape[0], sel.numel())
            for d, a in enumerate(coords):
                put(sel, np.clip(pts[which, d] + mrng.normal(0, spread, sel.numel()), 0.0, 1.0 - 1e-9), a)
        else:
            raise ValueError(kind)


def _cloud(n, seed):
    rng = np.random.default_rng(seed)
    centers = rng.uniform(0.2, 0.8, (5, 3))
    pos = np.where(rng.uniform(size=(n, 1)) < 0.5, rng.uniform(0, 1, (n, 3)),
                   centers[rng.integers(0, 5, n)] + rng.normal(0, 0.03, (n, 3)))
    return np.clip(pos, 0.0, 1.0 - 1e-6)


def _lattice(side):
    g = (np.arange(side) + 0.5) / side
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3))


# (name, key bits, bucket_focus, curve, positions, moves in front of syncs 2, 3, ...; moves after which the re-sort may be
#  given up -- too many movers or a leaf beyond the limit -- and with it the syncs it then backs off for)
_QUIET = ["none", "jitter", "few", "drift", "jitter"]
_CASES = [
    # fewer leaves than waves; one tile; two tiles with a short last one
    ("n65", 64, 64, 1, lambda: _cloud(65, 1), _QUIET, ()),
    ("n200", 64, 64, 1, lambda: _cloud(200, 2), _QUIET, ()),
    ("n700", 64, 64, 1, lambda: _cloud(700, 3), _QUIET, ()),
    ("n4200", 64, 64, 1, lambda: _cloud(4200, 4), _QUIET, ()),
    # 64, 32 and 16 leaves per tile; leaves just under the limit of 256 slots
    # (leaves of 8: a drift of 2e-3 is a good part of a leaf's width there, too many change their leaf for a re-sort)
    ("bucket8", 64, 8, 1, lambda: _cloud(20_000, 5), ["none", "jitter", "few", "jitter", "few"], ()),
    ("bucket100", 64, 100, 1, lambda: _cloud(20_000, 6), _QUIET, ()),
    ("bucket150", 64, 150, 1, lambda: _cloud(20_000, 7), _QUIET, ()),
    ("bucket200", 64, 200, 1, lambda: _cloud(20_000, 8), _QUIET, ()),
    # (full leaves hold 255 particles: one arrival is one too many, so only the syncs in front of the first move count)
    ("bucket255", 64, 255, 1, lambda: _cloud(20_000, 8), ["none", "jitter", "few", "jitter"], ("jitter",)),
    # step kinds side by side inside a quarter
    ("collapse", 64, 64, 1, lambda: _cloud(20_000, 9), ["none", "jitter", "collapse", "jitter", "few"], ("collapse",)),
    ("gather", 64, 64, 1, lambda: _cloud(20_000, 9), ["jitter", "gather", "jitter", "gather", "drift"], ()),
    ("drain", 64, 64, 1, lambda: _cloud(20_000, 10), ["none", "few", "many", "jitter", "few"], ("many",)),
    ("lattice", 64, 64, 1, lambda: _lattice(16), ["none", "few", "jitter", "few", "drift"], ()),
    ("keys32", 32, 64, 1, lambda: _cloud(20_000, 11), _QUIET, ()),
    ("morton", 64, 64, 0, lambda: _cloud(20_000, 12), _QUIET, ()),
]


@pytest.mark.gpu
@pytest.mark.parametrize("pairs", ["0", "1"])
@pytest.mark.parametrize("name,kb,bucket_focus,curve,positions,moves,may_give_up", _CASES, ids=[c[0] for c in _CASES])
def test_leaf_pass_equals_full_sort(hip, monkeypatch, pairs, name, kb, bucket_focus, curve, positions, moves, may_give_up):
    monkeypatch.setenv("CSTONE_RESORT_PAIRS", pairs)
    pos = positions()
    sa_, sb_ = (_Stepper(hip, kb, bucket_focus, curve, pos, 77, allow) for allow in (True, False))
    dom_a, dom_b = sa_.dom, sb_.dom
    kdt = np.uint64 if kb == 64 else np.uint32
    gave_up = False
    for step, kind in enumerate(["none"] + moves):
        if step:
            sa_.move(kind, np.random.default_rng(1000 + step))
            sb_.move(kind, np.random.default_rng(1000 + step))
        before = dom_a.stats()["resorts"]
        a, b = sa_.sync(), sb_.sync()
        va, vb = a["view"], b["view"]
        assert (va.end_index, va.num_focus_leaves) == (vb.end_index, vb.num_focus_leaves), (step, kind)
        for f in ("keys", "x", "y", "z", "h", "ident"):
            assert np.array_equal(a[f], b[f]), (step, kind, f)
        m, L = va.end_index, va.num_focus_leaves
        assert np.array_equal(dom_a.fetch(va.sfc_order, m, np.uint32), dom_b.fetch(vb.sfc_order, m, np.uint32)), (step, kind)
        assert np.array_equal(dom_a.fetch(va.layout, L + 1, np.uint32), dom_b.fetch(vb.layout, L + 1, np.uint32)), (step, kind)
        assert np.array_equal(dom_a.fetch(va.focus_leaves, L + 1, kdt), dom_b.fetch(vb.focus_leaves, L + 1, kdt)), (step, kind)
        assert np.array_equal(dom_a.fetch(va.focus_leaf_counts, L, np.uint32),
                              dom_b.fetch(vb.focus_leaf_counts, L, np.uint32)), (step, kind)
        assert np.all(a["keys"].view(kdt)[1:] >= a["keys"].view(kdt)[:-1]), (step, kind)
        # a sync that fell back to the full sort has not run the kernel: every sync behind the first re-sorts, except from
        # a move that is allowed to overflow onwards
        gave_up = gave_up or kind in may_give_up
        st = dom_a.stats()
        print(f"{name} pairs={pairs} sync {step} after '{kind}': resorts {st['resorts']} fallbacks {st['resort_fallbacks']} "
              f"movers {st['last_movers']} leaves {L}")
        if step and not gave_up:
            assert dom_a.stats()["resorts"] == before + 1, (step, kind, dom_a.stats())
    assert dom_b.stats()["resorts"] == 0
    assert dom_a.stats()["resorts"] >= 1, dom_a.stats()
