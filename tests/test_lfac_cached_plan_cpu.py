"""CPU: the two launch plans of a shape in csrc/lfac.hip.  A handle with an attached QP keeps the accumulators of the Schur complement's equality stages in a buffer E
(DESIGN 5.0000000): the FULL plan (first stage 0) is what every handle ran before and what a capture run takes, storing each tile's accumulator when it passes stage `cut`;
the CACHED plan starts every tile at `cut` from E.  Both must give every tile of real rows its stages exactly once and in order, with the flags the kernel acts on
(LItem::c: 1 first slice, 2 epilogue, 4 from E), and the full plan must still be the plan of the parent commit."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LKT, TT = 32, 64

# (nx, ne, nc): the four shapes of tests/test_gpu_schur_cache.py and C3
SHAPES = [(1000, 40, 0), (1024, 64, 32), (1100, 33, 17), (1300, 700, 300), (2500, 1500, 1000)]


def padded(nx):
    return (nx + 511) // 512 * 512 if nx > 512 else nx


@pytest.fixture(scope="module")
def L():
    lib = ctypes.CDLL(os.path.join(ROOT, "calipso.jl_amd", "libcalipso_hip.so"))
    lib.calipso_hip_debug_lfac_plan.argtypes = [ctypes.c_int32] * 4 + [ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_int32]
    lib.calipso_hip_debug_lfac_plan.restype = ctypes.c_int32
    lib.calipso_hip_debug_lfac_plan_items.argtypes = [ctypes.c_int32] * 5 + [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    lib.calipso_hip_debug_lfac_plan_items.restype = ctypes.c_int32
    return lib


_plans = {}


def plan_items(L, shape, first):
    """(items as an n x 9 array [launch, kind, i, j, a, b, c, pad0, pad1], [nst0, nst, cut, W]); scanned once per (shape, first) and shared"""
    key = (shape, first)
    if key not in _plans:
        nx, ne, nc = shape
        info = np.zeros(4, dtype=np.int32)
        n = L.calipso_hip_debug_lfac_plan_items(padded(nx) // TT, nx, ne, nc, first, None, 0, info.ctypes.data)
        assert n > 0, (shape, first)
        out = np.zeros((n, 9), dtype=np.int16)
        assert L.calipso_hip_debug_lfac_plan_items(padded(nx) // TT, nx, ne, nc, first, out.ctypes.data, n, info.ctypes.data) == n
        _plans[key] = (out, [int(v) for v in info])
    return _plans[key]


def cut_of(shape):
    nx, ne, nc = shape
    nst0 = (ne + LKT - 1) // LKT
    nst = nst0 + (nc + LKT - 1) // LKT
    return min(nst0, nst - 1), nst0, nst


def schur_slices(items, nblk):
    """tile -> its SCHUR slices in launch order, the parts of a split slice merged: [(launch, a, b, c)]"""
    per = {}
    for launch, kind, i, j, a, b, c, pad0, pad1 in items.tolist():
        if kind != 0:
            continue
        assert 0 <= j <= i < nblk
        per.setdefault((i, j), {}).setdefault(launch, []).append((a, b, c, pad0, pad1))
    out = {}
    for tile, by_launch in per.items():
        sl = []
        for launch in sorted(by_launch):
            parts = by_launch[launch]
            a, b, c, P, _ = parts[0]
            assert P in (1, 2, 4) and len(parts) == P, (tile, launch, parts)                    # ONE slice per tile and launch, split over P workgroups ...
            assert sorted(p[4] for p in parts) == list(range(P)), (tile, launch, parts)         # ... each with rows of its own ...
            assert all(p[:4] == (a, b, c, P) for p in parts), (tile, launch, parts)             # ... of the same stages, with the same flags
            sl.append((launch, a, b, c))
        out[tile] = sl
    return out


@pytest.mark.parametrize("cached", [False, True], ids=["full", "cached"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d_%d_%d" % s)
def test_every_real_tile_gets_its_stages_once_and_in_order(L, shape, cached):
    nx, ne, nc = shape
    cut, nst0, nst = cut_of(shape)
    assert 1 <= cut < nst
    first = cut if cached else 0
    items, info = plan_items(L, shape, first)
    assert info[:3] == [nst0, nst, cut]
    nblk = padded(nx) // TT
    slices = schur_slices(items, nblk)
    real = {(i, j) for j in range(nblk) for i in range(j, nblk) if i * TT < nx}
    assert set(slices) == real                                                                  # tiles of the padding alone have nothing to accumulate
    for tile, sl in slices.items():
        assert sl[0][1] == first and sl[-1][2] == nst, (tile, sl)
        for (l0, a0, b0, c0), (l1, a1, b1, c1) in zip(sl, sl[1:]):
            assert l0 < l1 and b0 == a1, (tile, sl)                                             # ascending, no gap, no overlap
        for q, (launch, a, b, c) in enumerate(sl):
            assert a < b and c & ~7 == 0
            assert (c & 1 != 0) == (q == 0), (tile, sl)                                         # the first slice starts the accumulator ...
            assert (c & 4 != 0) == (q == 0 and cached), (tile, sl)                              # ... from E in the cached plan, from zero in the full one
            assert (c & 2 != 0) == (q == len(sl) - 1), (tile, sl)                               # the last one adds Lxx and the regularisation
            # the products are complete before the launch that consumes the tile: -1 for tile (0, 0), else max(0, j - 2) (the head is launch -2)
            assert launch < (-1 if tile == (0, 0) else max(0, tile[1] - 2)), (tile, sl)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d_%d_%d" % s)
def test_a_capture_run_stores_every_tile_once_and_only_at_the_cut(L, shape):
    """k_lfac stores a slice's accumulator to E where a capture run's slice [a, b) has a < cut <= b, behind stage cut - 1 (item_schur): in the full plan that is ONE slice
    per real tile — so E holds every tile's sum over exactly the stages [0, cut), the ones the cached plan leaves out"""
    cut, nst0, nst = cut_of(shape)
    for tile, sl in schur_slices(plan_items(L, shape, 0)[0], padded(shape[0]) // TT).items():
        stores = [(a, b) for _, a, b, _ in sl if a < cut <= b]
        assert len(stores) == 1, (tile, sl)
    for tile, sl in schur_slices(plan_items(L, shape, cut)[0], padded(shape[0]) // TT).items():
        assert all(a >= cut for _, a, b, _ in sl), (tile, sl)                                   # nothing of the cached plan would store


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d_%d_%d" % s)
def test_the_full_plan_is_the_plan_of_the_parent(L, shape):
    """tests/golden/lfac_plan_first_stage0.json: what calipso_hip_debug_lfac_plan wrote for these shapes before the planner took a first stage.  The items the new export
    gives for first stage 0 are that plan's (per launch: items, SCHUR, FAR, ROW)."""
    nx, ne, nc = shape
    nblk = padded(nx) // TT
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "lfac_plan_first_stage0.json")))["plans"]["%d,%d,%d,%d" % (nblk, nx, ne, nc)]
    out = np.zeros(6 * 256)
    n = L.calipso_hip_debug_lfac_plan(nblk, nx, ne, nc, 0.0, 0.0, out.ctypes.data, 256)
    assert n == golden["launches"] == nblk + 1
    assert hashlib.sha256(out.tobytes()).hexdigest() == golden["sha256"]
    items, _ = plan_items(L, shape, 0)
    per_launch = out[:6 * n].reshape(n, 6)
    for l in range(n):
        mine = items[items[:, 0] == l - 2]
        assert [len(mine)] + [int((mine[:, 1] == k).sum()) for k in range(3)] == [int(v) for v in per_launch[l, 1:5]], l


def test_a_first_stage_beyond_the_last_has_no_plan(L):
    info = np.zeros(4, dtype=np.int32)
    assert L.calipso_hip_debug_lfac_plan_items(16, 1000, 40, 0, 2, None, 0, info.ctypes.data) == 0      # nst = 2: a tile with no stage left would get no epilogue
