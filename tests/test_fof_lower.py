"""cstone_hip_fof_lower_labels, the device step of a round of friends-of-friends across ranks, on its own:
labels[k] = min{ labels[m] : component[m] == component[k] } and the count of the lowered labels of a window, == a numpy
model.  Component patterns put one, seven or sixty-four distinct components into a wave, aligned to the waves and not;
label patterns differ only above or only below bit 32, so that a minimum taken on 32 bits fails."""
import numpy as np
import pytest

SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
COMPONENTS = ["singletons", "one", "runs64", "runs64-shifted", "mod7", "random"]
LABELS = ["random", "high-only", "low-only"]


def components(kind, n):
    k = np.arange(n)
    if kind == "singletons":
        c = np.random.default_rng(1).permutation(n)
    elif kind == "one":
        c = np.full(n, n // 2)
    elif kind == "runs64":
        c = (k // 64) * 64
    elif kind == "runs64-shifted":
        c = np.minimum(((k + 63) // 64) * 64, n - 1)  # runs of 64 that start one past the waves' first lanes
    elif kind == "mod7":
        c = k % 7
    else:
        c = np.random.default_rng(2).integers(0, max(n // 5, 1), n)
    assert c.min() >= 0 and c.max() < n
    return c.astype(np.uint32)


def labels_of(kind, n):
    rng = np.random.default_rng(3)
    if kind == "random":
        return rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    if kind == "high-only":  # equal low words: only the bits above 32 tell the values apart
        return (rng.integers(0, 2 ** 31, n, dtype=np.uint64) << np.uint64(32)) | np.uint64(0x89ABCDEF)
    return np.uint64(0xFEDCBA98) << np.uint64(32) | rng.integers(0, 2 ** 32, n, dtype=np.uint64)


def model(comp, labels, first, last):
    low = np.full(comp.size, np.iinfo(np.uint64).max, dtype=np.uint64)
    np.minimum.at(low, comp, labels)
    new = low[comp]
    return new, int((new[first:last] < labels[first:last]).sum())


def windows(n):
    w = [(0, n), (min(1, n), max(n - 1, min(1, n))), (n // 2, n // 2)]
    if n >= 128:
        w.append((64, 128))
    return w


def test_the_model_on_a_hand_made_case():
    comp = np.array([2, 0, 2, 0, 4], dtype=np.uint32)
    lab = np.array([9, 2 ** 40 + 1, 7, 2 ** 40, 5], dtype=np.uint64)
    new, changed = model(comp, lab, 0, 5)
    assert new.tolist() == [7, 2 ** 40, 7, 2 ** 40, 5] and changed == 2
    assert model(comp, lab, 1, 1)[1] == 0 and model(comp, lab, 1, 4)[1] == 1
    for kind in LABELS:  # a minimum on the low or the high words alone picks another element
        v = labels_of(kind, 1000)
        assert np.unique(v).size == v.size
    assert np.unique(labels_of("high-only", 1000) & np.uint64(0xFFFFFFFF)).size == 1
    assert np.unique(labels_of("low-only", 1000) >> np.uint64(32)).size == 1
    assert np.argmin(labels_of("random", 1000)) != np.argmin(labels_of("random", 1000) & np.uint64(0xFFFFFFFF))


def _dev(a):
    import torch

    return torch.from_numpy(a.view(np.int32 if a.dtype == np.uint32 else np.int64).copy()).cuda()


def _call(hip, comp, labels, changed, first, last, n=None):
    return hip.lib.cstone_hip_fof_lower_labels(hip.h, comp.data_ptr() if comp is not None else None,
                                               labels.numel() if n is None else n, first, last,
                                               labels.data_ptr() if labels is not None else None,
                                               changed.data_ptr() if changed is not None else None)


@pytest.mark.gpu
@pytest.mark.parametrize("lab", LABELS)
@pytest.mark.parametrize("kind", COMPONENTS)
def test_hip_lowering_equals_numpy(hip, kind, lab):
    """every size and window: labels == the model, `changed` grows by the model's count on top of what it held, and a
    second call on the result adds 0"""
    import torch

    for n in SIZES:
        comp, labels = components(kind, n), labels_of(lab, n)
        d_comp = _dev(comp)
        for first, last in windows(n):
            want, count = model(comp, labels, first, last)
            d_labels = _dev(labels)
            changed = torch.tensor([1000], dtype=torch.int32, device="cuda")
            assert _call(hip, d_comp, d_labels, changed, first, last) == 0
            assert _call(hip, d_comp, d_labels, changed, first, last) == 0  # (on the result: nothing drops any more)
            hip.sync()
            got = d_labels.cpu().numpy().view(np.uint64)
            assert np.array_equal(got, want), (n, first, last, np.flatnonzero(got != want)[:5])
            assert int(changed.item()) == 1000 + count, (n, first, last)


@pytest.mark.gpu
def test_hip_lowering_through_the_binding_and_in_many_blocks(hip):
    """Context.fof_lower_labels on 100 000 labels (hundreds of blocks) whose components are spread over the whole array"""
    import torch

    n = 100_003
    comp = np.random.default_rng(5).integers(0, n, n).astype(np.uint32)
    labels = labels_of("low-only", n)
    want, count = model(comp, labels, 10, n - 10)
    d_labels, changed = _dev(labels), torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.fof_lower_labels(_dev(comp), d_labels, changed, 10, n - 10)
    hip.sync()
    assert np.array_equal(d_labels.cpu().numpy().view(np.uint64), want) and int(changed.item()) == count


@pytest.mark.gpu
def test_hip_lowering_refuses_bad_arguments(hip):
    """null pointers, last < first and last > n: CSTONE_E_ARG, labels and `changed` untouched; n == 0 is fine"""
    import torch

    n = 300
    comp, labels = components("mod7", n), labels_of("random", n)
    d_comp, d_labels = _dev(comp), _dev(labels)
    changed = torch.tensor([7], dtype=torch.int32, device="cuda")
    E_ARG = -1
    assert _call(hip, None, d_labels, changed, 0, n) == E_ARG
    assert _call(hip, d_comp, None, changed, 0, n, n=n) == E_ARG
    assert _call(hip, d_comp, d_labels, None, 0, n) == E_ARG
    assert _call(hip, d_comp, d_labels, changed, 5, 4) == E_ARG
    assert _call(hip, d_comp, d_labels, changed, 0, n + 1) == E_ARG
    assert hip.lib.cstone_hip_fof_lower_labels(None, d_comp.data_ptr(), n, 0, n, d_labels.data_ptr(), changed.data_ptr()) == E_ARG
    assert _call(hip, d_comp, d_labels, changed, 0, 0, n=0) == 0
    hip.sync()
    assert np.array_equal(d_labels.cpu().numpy().view(np.uint64), labels) and int(changed.item()) == 7
    assert hip.lib.cstone_hip_last_error(hip.h)
