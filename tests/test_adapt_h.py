"""Adaptive smoothing lengths (csrc/adapt_h.hip, cstone_hip_adapt_smoothing_lengths and the two domain calls): h iterated
per particle to a neighbour count of ng0 +- tol inside one kernel.

The reference is the restatement of the rule in tests/adapt_h_support.py: numpy in the coordinate type, the count of an
iteration taken from the oracle's walk (the one tests/test_neighbors.py proves equal to the kernel's walk).  The CPU tests
establish that it may serve: its counts equal a brute force at every iteration's h for the seeds used here (a difference
would be a node pruned by rounding: not tolerated away), and its results have the properties the rule promises.  The GPU
tests compare h, counts and status of the kernel with it bit for bit, on outputs pre-filled with a sentinel.

Every shape asserts, from the restatement, the premise that makes it exercise its branch."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import adapt_h_support as ah
from adapt_h_support import CAPPED, FLAGS, INF, NOT_CONVERGED, STALLED, WALKS, Params
from neighbors_support import SENT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RBS = [32, 64]
ALL_SHAPES = ["uniform", "clumps"] + ah.GPU_SHAPES
NEW_SYMBOLS = ("cstone_hip_adapt_smoothing_lengths", "cstone_hip_domain_adapt_h", "cstone_hip_domain_mr_adapt_h")


def walks_of(status):
    return (status & WALKS).astype(np.int64)


def flagged(status):
    return (status & FLAGS) != 0


def check_premise(name, rb):
    """what makes the shape exercise the code it is here for, from the restatement"""
    s, r = ah.shape(name, rb), ah.result(name, rb)
    case, p, kind = s.case, s.params, name.split("-")[0]
    w, st = walks_of(r.status), r.status
    rows = np.arange(s.first, s.last)
    assert s.first % 64 != 0 or kind in ("tiny", "uneven", "uniform", "clumps")
    if name == "tiny-n1":
        assert case.n == 1 and p.max_iter == 3 and p.grow_limit == INF
        assert [c.tolist() for _, _, c in r.trace] == [[0]] * 4 and st[0] == (4 | NOT_CONVERGED)
    elif name == "tiny-n2":
        assert case.n == 2 and (w > 1).all() and not flagged(st).any()
    elif kind == "tiny":
        assert case.o["num_nodes"] == 1 and case.n == 65 and w.max() >= 3 and w.min() < w.max()  # one leaf, two waves
    elif kind == "range":
        assert s.last - s.first == int(name.split("-")[1]) and case.n == 600 and w.max() > 1
    elif kind == "uneven":
        waves = [w[k:k + 64] for k in range(0, w.size, 64)]
        assert any(v.min() == 1 and v.max() >= 4 for v in waves)  # a lane with one walk beside one with four
        assert any(v.max() == 1 and not flagged(st[64 * k:64 * k + 64]).any() for k, v in enumerate(waves))
    elif kind == "fold":
        assert 1 in case.box.bc
        before, after = ah.cube_inside(case, rows, case.h[rows]), ah.cube_inside(case, rows, r.h[rows])
        assert (before & ~after).any()  # the fold switches on between the first and the last walk
    elif kind == "long":
        big = case.leaf_counts.max()
        assert big > 128 if "clustered" in name else big in range(300, 320)
        assert w.max() > 1
    elif name == "edge-tol0":
        assert p.tol == 0 and (st & NOT_CONVERGED).any() and (~flagged(st)).any()
    elif name == "edge-toomany":
        assert p.ng0 > case.n - 1 and p.grow_limit == INF and ((st & FLAGS) == NOT_CONVERGED).all()
    elif name == "edge-toomanycapped":
        assert p.ng0 > case.n - 1 and ((st & FLAGS) == CAPPED).all()
    elif name == "edge-grow1":
        assert (r.h[rows] <= case.h[rows]).all() and (st & CAPPED).any() and (r.h[rows] < case.h[rows]).any()
    elif name == "edge-growinf":
        assert p.grow_limit == INF and (r.h[rows] > 2 * case.h[rows]).sum() == 0 and not (st & CAPPED).any()
    elif name == "edge-iter0":
        assert p.max_iter == 0 and (w == 1).all() and (st & NOT_CONVERGED).any()


# ---- CPU: the restatement may serve as the reference ----------------------------------------------------------------

def test_header_declares_and_the_bindings_export_the_three_calls():
    import cstone_amd

    text = open(os.path.join(ROOT, "include", "cstone_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(cstone_hip_\w+)\s*\(", text))
    lib = cstone_amd.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared and name in cstone_amd.EXPORTS and hasattr(lib, name), name
    assert cstone_amd.STAGES["adapt_h"] == int(re.search(r"#define CSTONE_STAGE_ADAPT_H (\d+)", text).group(1))
    for macro, value in (("NOT_CONVERGED", NOT_CONVERGED), ("CAPPED", CAPPED), ("STALLED", STALLED)):
        assert int(re.search(rf"#define CSTONE_ADAPT_H_{macro} (0x[0-9a-fA-F]+)u", text).group(1), 16) == value
        assert getattr(cstone_amd, "ADAPT_H_" + macro) == value


@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("name", ALL_SHAPES)
def test_restated_counts_equal_brute_force_at_every_iteration(name, rb):
    if name in ah.GPU_SHAPES:
        check_premise(name, rb)
    s, r = ah.shape(name, rb), ah.result(name, rb)
    rows = np.arange(s.first, s.last)
    assert 1 <= len(r.trace) <= s.params.max_iter + 1
    for it, (hw, active, cnt) in enumerate(r.trace):
        brute = ah.brute_counts(s.case, rows[active], hw[active])
        assert np.array_equal(brute, cnt[active]), (name, it, np.flatnonzero(brute != cnt[active])[:8])


@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("name", ALL_SHAPES)
def test_flags_say_what_the_output_is(name, rb):
    """no flag <=> the count recomputed from the output h lies within ng0 +- tol; CAPPED => h == hcap bit for bit and
    too few neighbours; the counts are those of a fresh walk at the output h; h outside the range keeps its bits"""
    s, r = ah.shape(name, rb), ah.result(name, rb)
    case, p = s.case, s.params
    T = case.x.dtype.type
    fresh = ah.oracle_counts(case, r.h, s.first, s.last)
    assert np.array_equal(fresh, r.counts)
    within = np.abs(fresh - p.ng0) <= p.tol
    assert np.array_equal(~flagged(r.status), within)
    capped = (r.status & CAPPED) != 0
    with np.errstate(all="ignore"):
        hcap = case.h[s.first:s.last] * T(np.float32(p.grow_limit))
    assert np.array_equal(r.h[s.first:s.last][capped].view(np.uint8), hcap[capped].view(np.uint8))
    assert (fresh[capped] + p.tol < p.ng0).all()
    assert sum(((r.status & f) != 0).astype(int) for f in (NOT_CONVERGED, CAPPED, STALLED)).max() <= 1  # one reason
    outside = np.ones(case.n, dtype=bool)
    outside[s.first:s.last] = False
    assert np.array_equal(r.h[outside].view(np.uint8), case.h[outside].view(np.uint8))
    assert (walks_of(r.status) >= 1).all() and (walks_of(r.status) <= p.max_iter + 1).all()


@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("name", ["uniform", "clumps", "fold-111", "long-clump300", "edge-tol0"])
def test_a_second_run_keeps_what_had_converged(name, rb):
    s, r = ah.shape(name, rb), ah.result(name, rb)
    again = ah.adapt(s.case, s.first, s.last, s.params, h0=r.h)
    ok = ~flagged(r.status)
    assert ok.any()
    assert (again.status[ok] == 1).all()
    assert np.array_equal(again.h[s.first:s.last][ok].view(np.uint8), r.h[s.first:s.last][ok].view(np.uint8))
    assert np.array_equal(again.counts[ok], r.counts[ok])


@pytest.mark.parametrize("rb", RBS)
def test_no_iteration_is_a_plain_count(oracle, rb):
    s, r = ah.shape("edge-iter0", rb), ah.result("edge-iter0", rb)
    assert np.array_equal(r.h.view(np.uint8), s.case.h.view(np.uint8))
    assert np.array_equal(r.counts, s.case.find(oracle, s.first, s.last, 1)[1])


@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("name", ["uniform", "clumps"])
def test_the_rule_converges_on_ordinary_clouds(name, rb):
    """ng0 = 50, tol = 5, max_iter = 10, grow_limit = 2, h0 off by a factor in [0.6, 1.4]: at most 1 % of the targets end
    NOT_CONVERGED or STALLED (a condition on the inputs, not a tolerance of the kernel)"""
    s, r = ah.shape(name, rb), ah.result(name, rb)
    assert s.params == ah.STD and s.last - s.first == 3000
    lost = ((r.status & (NOT_CONVERGED | STALLED)) != 0).sum()
    print(f"{name} f{rb}: {lost} of 3000 not converged or stalled, {int((r.status & CAPPED != 0).sum())} capped, "
          f"mean walks {walks_of(r.status).mean():.2f}")
    assert lost <= 30
    assert 1.5 <= walks_of(r.status).mean() <= 5


# ---- GPU -------------------------------------------------------------------------------------------------------------

def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


class DevCase:
    """the arrays of a case on the device; h is uploaded anew for every call (the call overwrites it)"""

    PAD = 70  # rows of counts, status and lists behind the last target, to see that they stay untouched

    def __init__(self, hip, case):
        import cstone_amd

        self.hip, self.case = hip, case
        self.x, self.y, self.z = (_dev(a) for a in (case.x, case.y, case.z))
        self.co, self.i2l = _dev(case.o["child_offsets"]), _dev(case.o["internal_to_leaf"])
        self.layout, self.cen, self.siz = _dev(case.layout), _dev(case.cen), _dev(case.siz)
        self.cbox = cstone_amd.make_cbox(case.box.lim, case.box.bc)

    def call(self, first, last, p, ngmax=0, h=None, null=(), real_bits=None, expect=0):
        """one cstone_hip_adapt_smoothing_lengths on outputs pre-filled with the sentinel: (rc, h [n], counts, status,
        lists [rows, ngmax]) with PAD more rows than targets"""
        import torch

        hip, P = self.hip, lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        rows = max(last - first, 0) + self.PAD
        hd = _dev(self.case.h if h is None else h)
        cnt = torch.full((rows,), -1, dtype=torch.int32, device="cuda")
        st = torch.full((rows,), -1, dtype=torch.int32, device="cuda")
        lst = torch.full((rows * max(ngmax, 1),), -1, dtype=torch.int32, device="cuda")
        args = dict(ctx=hip.h, real_bits=C.c_int(self.case.rb if real_bits is None else real_bits), x=P(self.x),
                    y=P(self.y), z=P(self.z), h=P(hd), first=C.c_uint32(first), last=C.c_uint32(last),
                    box=C.byref(self.cbox), co=P(self.co), i2l=P(self.i2l), layout=P(self.layout), cen=P(self.cen),
                    siz=P(self.siz), ng0=C.c_uint32(p.ng0), tol=C.c_uint32(p.tol), max_iter=C.c_uint32(p.max_iter),
                    grow=C.c_float(p.grow_limit), ngmax=C.c_uint32(ngmax), lists=P(lst) if ngmax else None, counts=P(cnt),
                    status=P(st))
        for k in null:
            args[k] = None
        rc = hip.lib.cstone_hip_adapt_smoothing_lengths(*args.values())
        assert rc == expect, (rc, hip.lib.cstone_hip_last_error(hip.h))
        hip.sync()  # raises if the sticky device-side error word is set (a traversal stack overflow sets it)
        u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
        return hd.cpu().numpy(), u32(cnt), u32(st), u32(lst).reshape(rows, max(ngmax, 1))


def assert_equals_restatement(got, case, first, last, r, what):
    h, cnt, st, _ = got
    nt = last - first
    bad = np.flatnonzero(st[:nt] != r.status)
    assert bad.size == 0, (what, "status", bad[:8].tolist(), st[bad[:8]].tolist(), r.status[bad[:8]].tolist())
    bad = np.flatnonzero(cnt[:nt] != r.counts)
    assert bad.size == 0, (what, "counts", bad[:8].tolist(), cnt[bad[:8]].tolist(), r.counts[bad[:8]].tolist())
    assert h.dtype == r.h.dtype
    bad = np.flatnonzero(h.view(case.h.dtype.str.replace("f", "u")) != r.h.view(case.h.dtype.str.replace("f", "u")))
    assert bad.size == 0, (what, "h", bad[:8].tolist(), h[bad[:8]].tolist(), r.h[bad[:8]].tolist())
    assert (cnt[nt:] == SENT).all() and (st[nt:] == SENT).all(), (what, "written behind the last target")


@pytest.mark.gpu
@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("name", ah.GPU_SHAPES)
def test_hip_equals_the_restatement(hip, name, rb):
    """h (the whole array: outside the range it keeps its input bits), counts and status bit for bit, ngmax = 0 with a
    null list; the rows behind the last target keep the sentinel"""
    check_premise(name, rb)
    s, r = ah.shape(name, rb), ah.result(name, rb)
    d = DevCase(hip, s.case)
    got = d.call(s.first, s.last, s.params)
    w = walks_of(got[2][:s.last - s.first])
    print(f"{name} f{rb}: walks mean {w.mean():.2f} max {w.max()}, flagged {int(flagged(got[2][:s.last - s.first]).sum())}")
    assert_equals_restatement(got, s.case, s.first, s.last, r, name)


@pytest.mark.gpu
@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("name", ["range-257", "long-clump300", "fold-111"])
def test_hip_lists_are_those_of_find_neighbors_at_the_output_h(hip, oracle, name, rb):
    """ngmax below and above the counts: the lists equal the oracle's find_neighbors on the output h entry for entry, the
    sentinel is intact beyond min(count, ngmax); h, counts and status are what they are without lists"""
    s, r = ah.shape(name, rb), ah.result(name, rb)
    case, nt = s.case, s.last - s.first
    d = DevCase(hip, case)
    small, large = max(1, int(r.counts.min()) // 2), int(r.counts.max()) + 3
    assert small < r.counts.max()
    for ngmax in (small, large):
        got = d.call(s.first, s.last, s.params, ngmax=ngmax)
        assert_equals_restatement(got, case, s.first, s.last, r, (name, ngmax))
        ref_l = oracle.find_neighbors(case.x, case.y, case.z, r.h, s.first, s.last, case.box, case.o, case.layout,
                                      case.cen, case.siz, ngmax, 1.0)[0]
        stored = np.arange(ngmax)[None, :] < np.minimum(r.counts, ngmax)[:, None]
        lists = got[3]
        bad = np.flatnonzero(((lists[:nt] != ref_l) & stored).any(1))
        assert bad.size == 0, (name, ngmax, "rows", bad[:8].tolist())
        assert (lists[:nt][~stored] == SENT).all() and (lists[nt:] == SENT).all(), (name, ngmax, "beyond the count")


@pytest.mark.gpu
@pytest.mark.parametrize("rb", RBS)
def test_hip_is_repeatable_and_refuses_bad_arguments(hip, rb):
    """two identical calls give the same bits; every refusal is CSTONE_E_ARG with h, counts, status and lists untouched;
    an empty range is accepted and writes nothing"""
    s = ah.shape("range-257", rb)
    d = DevCase(hip, s.case)
    a, b = d.call(s.first, s.last, s.params, ngmax=4), d.call(s.first, s.last, s.params, ngmax=4)
    assert all(np.array_equal(u.view(np.uint8), v.view(np.uint8)) for u, v in zip(a, b))
    E_ARG, p = -1, s.params
    refusals = [dict(null=[k]) for k in ("ctx", "x", "y", "z", "h", "box", "co", "i2l", "layout", "cen", "siz", "counts",
                                         "status")]
    refusals += [dict(first=s.last, last=s.first), dict(real_bits=16), dict(p=p._replace(ng0=0)),
                 dict(p=p._replace(grow_limit=0.5)), dict(p=p._replace(grow_limit=float("nan"))),
                 dict(ngmax=4, null=["lists"])]
    for kw in refusals:
        kw = dict(dict(first=s.first, last=s.last, p=p), **kw)
        got = d.call(kw.pop("first"), kw.pop("last"), kw.pop("p"), expect=E_ARG, **kw)
        assert np.array_equal(got[0].view(np.uint8), s.case.h.view(np.uint8)), kw
        assert all((t == SENT).all() for t in got[1:]), kw
    got = d.call(100, 100, p, ngmax=4)
    assert np.array_equal(got[0].view(np.uint8), s.case.h.view(np.uint8)) and all((t == SENT).all() for t in got[1:])


class _Raw:
    """a device pointer of a domain view where the bindings expect a tensor"""

    def __init__(self, ptr):
        self.ptr = ptr

    def data_ptr(self):
        return self.ptr


@pytest.mark.gpu
@pytest.mark.parametrize("rb", RBS)
def test_hip_domain_adapt_h_is_the_kernel_level_call_on_the_view(hip, rb):
    """Domain.adapt_h after a sync = Context.adapt_smoothing_lengths on the view's octree and the synced arrays, bit for
    bit, with grow_limit 0 meaning no limit; before the first sync it is refused"""
    import torch

    import cstone_amd
    from cstone_amd.domain import Domain

    s = ah.shape("uniform", rb)
    case, p = s.case, Params(50, 5, 10, 0.0)
    tdt = torch.float32 if rb == 32 else torch.float64
    perm = np.random.default_rng(5).permutation(case.n)
    x, y, z, h = [torch.from_numpy(a[perm].copy()).cuda() for a in (case.x, case.y, case.z, case.h)]
    dom = Domain(hip, cstone_amd.HILBERT, 64, rb, 64, 16, 0.5, cstone_amd.make_cbox(case.box.lim, case.box.bc))
    with pytest.raises(cstone_amd.CstoneError):
        dom.adapt_h(x, y, z, h, p.ng0, p.tol, p.max_iter)
    keys = torch.zeros(case.n, dtype=torch.int64, device="cuda")
    scratch = [torch.empty(case.n, dtype=tdt, device="cuda") for _ in range(3)]
    keys, x, y, z, h, _, _ = dom.sync(keys, x, y, z, h, scratch)
    hip.sync()
    v = dom.view()
    assert (v.start_index, v.end_index) == (0, case.n)
    h2 = h.clone()
    cnt, st = dom.adapt_h(x, y, z, h, p.ng0, p.tol, p.max_iter)
    tree = dict(child_offsets=_Raw(v.child_offsets), internal_to_leaf=_Raw(v.internal_to_leaf))
    _, cnt2, st2 = hip.adapt_smoothing_lengths(x, y, z, h2, 0, case.n, v.box, tree, _Raw(v.layout), _Raw(v.centers),
                                               _Raw(v.sizes), p.ng0, p.tol, p.max_iter)
    hip.sync()
    assert torch.equal(cnt, cnt2) and torch.equal(st, st2) and torch.equal(h.view(torch.uint8), h2.view(torch.uint8))
    status = st.cpu().numpy().view(np.uint32)
    assert not flagged(status).all() and walks_of(status).max() > 1
    # the same cloud as the restatement's, in the domain's order (its box is measured, so its tree is another one): the
    # results agree wherever both walks equal the brute force, which is everywhere for this seed
    r = ah.adapt(case, 0, case.n, Params(50, 5, 10, INF))
    order = {(a, b, c): k for k, (a, b, c) in enumerate(zip(case.x.tolist(), case.y.tolist(), case.z.tolist()))}
    back = np.array([order[t] for t in zip(x.cpu().tolist(), y.cpu().tolist(), z.cpu().tolist())])
    assert np.array_equal(status, r.status[back]) and np.array_equal(h.cpu().numpy(), r.h[back])


def _launch(nproc, port, pbc, timeout=600):
    env = dict(os.environ, OMP_NUM_THREADS="2", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "adapt_h_mr_worker.py")]
    p = subprocess.run(cmd + (["--pbc"] if pbc else []), capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("ADAPT_RESULT ")]
    assert lines, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads(lines[-1][len("ADAPT_RESULT "):])
    print(json.dumps(res))
    assert p.returncode == 0 and res["ok"], str(res["bad"])[:3000] + p.stderr[-2000:]
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("pbc", [False, True], ids=["open", "pbc"])
@pytest.mark.parametrize("nproc", [2, 3])
def test_hip_adapt_h_on_several_ranks(nproc, pbc):
    """NativeDistributedDomain.adapt_h on 2 and 3 gloo ranks that share the GPU, 6 000 particles, halo factor 1.5: per
    particle (a global id travels as a property) h, count and status equal the restatement on the WHOLE cloud with
    grow_limit = 1.5 -- the halos cover the capped radius; a grow_limit of 2 and a second call before the next sync are
    refused; exchange=False leaves the halo ranges of h as they were, exchange=True fills them with the owners' new
    values (tests/adapt_h_mr_worker.py)"""
    res = _launch(nproc, 29930 + 2 * nproc + int(pbc), pbc)
    assert res["ranks"] == nproc and res["particles"] == 6000
    assert res["capped"] > 0 and res["converged"] > 3000 and res["max_walks"] >= 4
    assert all(hl > 0 for hl in res["halos"])


def _compile_example(exe):
    libdir = os.path.join(ROOT, "cornerstone-octree_amd", "lib")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Wno-comment", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "cornerstone-octree_amd", "include"),
                    os.path.join(ROOT, "examples", "adapt_h_example.cpp"), "-L", libdir, "-lcstone_hip",
                    f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)


def test_cpp_example_compiles_with_a_host_compiler(tmp_path):
    """examples/adapt_h_example.cpp (adaptSmoothingLengthsGpu, Domain::adaptSmoothingLengths and through it the
    MultiRankDomain method) against the C++ host layer, with g++"""
    _compile_example(tmp_path / "adapt_h_example")


@pytest.mark.gpu
def test_hip_cpp_example_runs(tmp_path):
    """sync, Domain::adaptSmoothingLengths, the four status totals"""
    exe = tmp_path / "adapt_h_example"
    _compile_example(exe)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout
    print(out)
    m = re.search(r"converged (\d+) not_converged (\d+) capped (\d+) stalled (\d+)", out)
    assert m, out
    tot = [int(v) for v in m.groups()]
    n = int(re.search(r"particles (\d+)", out).group(1))
    assert sum(tot) == n and tot[0] >= 0.9 * n
