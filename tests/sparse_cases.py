"""Step lists for the sparse-step integrator (adder_hip_integrate_sparse*, csrc/adder_sparse.hip) at its edges -- pure
numpy, shared by tests/test_sparse_edges_cpu.py (sim == oracle, every reach predicate) and tests/test_gpu_sparse_edges.py
(product == oracle).

A case names the edge it must reach and carries a predicate for it.  The predicate looks at the list the way the
kernels do: unit keys (invalid steps = 0xffffffff), stable argsort, runs of equal keys, 256 sorted positions per block.

The radix sort behind the integrator is rocPRIM's (hipcub::DeviceRadixSort::SortPairs), which picks one of three
algorithms by size (rocprim/device/device_radix_sort.hpp, radix_sort_impl; device_radix_sort_config.hpp):
    n <= block_size * items_per_thread = 256 * 4        one block sorts everything
    n <= merge_sort_limit = 1024 * 1024                 block sort + merge passes
    beyond                                              onesweep
"""
import functools

import numpy as np

from oracle import oracle as O

BLOCK_SORT_ITEMS = 256 * 4      # kernel_config<256, 4>, the single-block limit
MERGE_SORT_LIMIT = 1024 * 1024  # radix_sort_config<>::merge_sort_limit
GRID_BLOCK = 256                # threads per block of the keys / run / emit kernels
FIRST_WORKSPACE = 4096          # sparse_prepare: the first allocation is max(n, 4096) steps

REF_TIME = 20
INVALID = 0xFFFFFFFF
NO_SIDE, INTEGRATE_ONLY, TEST_ONLY, FLUSH = 1, 2, 4, 8  # ADDER_SPARSE_* (include/adder_hip.h)
# every defined value of AdderSparseStep::pad: the side-plane bit with at most one of the DAVIS source's partial steps
# (the three are alternatives: the header defines no meaning for two of them at once)
PADS = np.array([k | s for k in (0, INTEGRATE_ONLY, TEST_ONLY, FLUSH) for s in (0, NO_SIDE)], np.uint16)
_PAD_WEIGHTS = np.array([4, 4, 2, 2, 2, 2, 1, 1], float) / 18.0


def sort_path(n):
    return "block" if n <= BLOCK_SORT_ITEMS else "merge" if n <= MERGE_SORT_LIMIT else "onesweep"


# ---------------------------------------------------------------------------------------------------------------
# the list as the kernels see it
# ---------------------------------------------------------------------------------------------------------------
def unit_keys(st, W, Cn, row_begin, rows):
    """adder_sparse_keys_kernel: the unit of every step, INVALID for a step outside the band / plane."""
    x, y = st["x"].astype(np.int64), st["y"].astype(np.int64)
    c = np.where(st["c"] == 0xFF, 0, st["c"]).astype(np.int64)
    ok = (x < W) & (y >= row_begin) & (y - row_begin < rows) & (c < Cn)
    return np.where(ok, ((y - row_begin) * W + x) * Cn + c, INVALID).astype(np.uint32)


def sorted_view(st, W, Cn, row_begin, rows):
    """(sorted keys, the step index at every sorted position): a stable sort, invalid steps last."""
    keys = unit_keys(st, W, Cn, row_begin, rows)
    order = np.argsort(keys, kind="stable")
    return keys[order], order


def runs(sorted_keys):
    """(start position, length, key) of every run of equal keys, invalid steps included as the last run."""
    n = len(sorted_keys)
    if n == 0:
        z = np.zeros(0, np.int64)
        return z, z, np.zeros(0, np.uint32)
    starts = np.flatnonzero(np.r_[True, sorted_keys[1:] != sorted_keys[:-1]])
    return starts, np.diff(np.r_[starts, n]), sorted_keys[starts]


# ---------------------------------------------------------------------------------------------------------------
# contents of a step, given its unit
# ---------------------------------------------------------------------------------------------------------------
def steps_on(rng, units, W, Cn, row_begin=0):
    """Steps on the given units, in the given order.  As test_device_logic_cpu._sparse_steps, plus what it leaves out:
    times that are no multiple of ref_time (0.37 and 2.5 of it), intensities that are not val * span, a zero time on
    some test-only steps, and every defined pad value."""
    units = np.asarray(units, np.int64)
    n = len(units)
    st = np.zeros(n, O.SPARSE_STEP_DTYPE)
    st["x"] = (units // Cn) % W
    st["y"] = (units // Cn) // W + row_begin
    st["c"] = 0xFF if Cn == 1 else units % Cn
    val = rng.choice(np.array([0, 1, 3, 9, 40, 128, 200, 255]), n)
    span = rng.choice(np.array([1, 1, 1, 2, 5, 40, 700, 0.37, 2.5]), n)
    st["frame_val"] = val
    st["pad"] = rng.choice(PADS, n, p=_PAD_WEIGHTS)
    st["intensity"] = (val * span + rng.choice(np.array([0.0, 0.0, 0.25, 0.625, 1.0 / 3.0, 17.3]), n)).astype(np.float32)
    st["time"] = (span * REF_TIME).astype(np.float32)
    st["time"][((st["pad"] & TEST_ONLY) != 0) & (rng.random(n) < 0.5)] = 0.0
    return st


def random_units(rng, n_units, n, hot=0.3):
    """A few hot units fire again and again, the rest anywhere."""
    hotu = rng.integers(0, n_units, max(2, int(n_units * 0.05)))
    return np.where(rng.random(n) < hot, hotu[rng.integers(0, len(hotu), n)], rng.integers(0, n_units, n))


class Case:
    """One context and the calls made on it.  `build(rng)` -> list of step arrays; `reach(case)` -> bool.
    Oracle and sim planes are (W, rows, Cn) at row_begin; the product's is (W, height, Cn) with the band given."""

    def __init__(self, name, edge, build, reach, *, W=37, rows=23, Cn=1, row_begin=0, height=None, multi_mode=O.NORMAL,
                 time_mode=O.DELTA_T, delta_t_max=160, max_depth=16, crf=(7, 7), start_frames=2, exact_cap=False,
                 quality_change=None, seed=0):
        self.name, self.edge, self._build, self._reach = name, edge, build, reach
        self.W, self.rows, self.Cn, self.row_begin = W, rows, Cn, row_begin
        self.height = rows + row_begin if height is None else height
        self.multi_mode, self.time_mode, self.delta_t_max, self.max_depth = multi_mode, time_mode, delta_t_max, max_depth
        self.crf, self.start_frames, self.exact_cap = crf, start_frames, exact_cap
        self.quality_change = quality_change  # (before call index, c_thresh_max, velocity, delta_t_max, baseline)
        self.seed = seed
        self.n_units = W * rows * Cn

    @functools.cached_property
    def calls(self):
        return self._build(self, np.random.default_rng(self.seed))

    def view(self, k):
        return sorted_view(self.calls[k], self.W, self.Cn, self.row_begin, self.rows)

    def reached(self):
        return bool(self._reach(self))

    def rand(self, rng, n, hot=0.3):
        return steps_on(rng, random_units(rng, self.n_units, n, hot), self.W, self.Cn, self.row_begin)

    def __repr__(self):
        return self.name


def _all_valid(case, k):
    keys, _ = case.view(k)
    return len(keys) == 0 or keys[-1] != INVALID


# ---------------------------------------------------------------------------------------------------------------
# 1. grid and sort paths
# ---------------------------------------------------------------------------------------------------------------
def _grid_case(n, seed):
    def build(case, rng):  # n steps on a fresh context (the first workspace), state in between, n steps again
        return [case.rand(rng, n), case.rand(rng, 1500), case.rand(rng, n)]

    def reach(case):
        blocks = (n + GRID_BLOCK - 1) // GRID_BLOCK
        want_path = "block" if n <= 1024 else "merge"
        want_blocks = {1: 1, 255: 1, 256: 1, 257: 2, 1024: 4, 1025: 5}[n]
        return (len(case.calls[0]) == n == len(case.calls[2]) and blocks == want_blocks and sort_path(n) == want_path
                and _all_valid(case, 0) and _all_valid(case, 2))

    return Case(f"grid_n{n}", f"{n} steps: grid of {(n + 255) // 256} block(s), {sort_path(n)} sort", build, reach,
                multi_mode=(O.NORMAL, O.COLLAPSE)[seed & 1], time_mode=(O.DELTA_T, O.ABSOLUTE_T)[(seed >> 1) & 1], seed=100 + seed)


def _big_case(n, path, seed, mm, tm):
    def build(case, rng):
        return [case.rand(rng, n, hot=0.05)]

    def reach(case):
        keys, _ = case.view(0)
        _, lens, _ = runs(keys)
        return (sort_path(n) == path and len(keys) == n and keys[-1] != INVALID and len(lens) == case.n_units
                and n // case.n_units >= 512 and lens.min() >= 256)

    return Case(f"big_n{n}", f"{n} steps, about 512 per unit: the {path} sort", build, reach, W=64, rows=32,
                multi_mode=mm, time_mode=tm, exact_cap=True, seed=seed)


# ---------------------------------------------------------------------------------------------------------------
# 3. runs
# ---------------------------------------------------------------------------------------------------------------
def _shuffled(rng, units):
    return rng.permutation(np.asarray(units, np.int64))


def _with_state(build_one):
    def build(case, rng):  # the constructed list on a fresh context, random steps, the constructed list on that state
        a = build_one(case, rng)
        return [a, case.rand(rng, 1000), build_one(case, rng)]
    return build


def _run_crosses_block():
    def one(case, rng):  # units 0..254 once each, then unit 255 forty times: its run starts at sorted position 255
        return steps_on(rng, _shuffled(rng, np.r_[np.arange(255), np.full(40, 255), rng.integers(256, case.n_units, 300)]),
                        case.W, case.Cn, case.row_begin)

    def reach(case):
        ok = True
        for k in (0, 2):
            keys, _ = case.view(k)
            starts, lens, _ = runs(keys)
            ok = ok and bool(np.any((starts % GRID_BLOCK == GRID_BLOCK - 1) & (lens >= 2))) and keys[-1] != INVALID
        return ok

    return Case("run_crosses_block", "a run that starts at sorted position 255 (mod 256) and goes on in the next block",
                _with_state(one), reach, multi_mode=O.COLLAPSE, time_mode=O.ABSOLUTE_T, seed=201)


def _long_runs():
    def build(case, rng):
        hot = 411
        a = steps_on(rng, _shuffled(rng, np.r_[np.full(300, hot), rng.integers(0, case.n_units, 700)]), case.W, case.Cn)
        b = steps_on(rng, np.full(3000, hot), case.W, case.Cn)
        return [a, b, case.rand(rng, 500)]

    def reach(case):
        k0, _ = case.view(0)
        k1, _ = case.view(1)
        _, lens0, _ = runs(k0)
        _, lens1, keys1 = runs(k1)
        return lens0.max() >= 300 and len(lens1) == 1 and lens1[0] == 3000 == len(case.calls[1]) and keys1[0] != INVALID

    return Case("long_runs", "one unit with 300 steps of a call; 3000 steps that are all of a call", build, reach,
                multi_mode=O.NORMAL, time_mode=O.ABSOLUTE_T, seed=202)


def _reverse_raster():
    def one(case, rng):
        return steps_on(rng, np.arange(case.n_units)[::-1], case.W, case.Cn)

    def reach(case):
        keys, order = case.view(0)
        n = case.n_units
        return (np.array_equal(keys, np.arange(n)) and np.array_equal(order, np.arange(n)[::-1])
                and np.array_equal(unit_keys(case.calls[2], case.W, case.Cn, 0, case.rows), np.arange(n)[::-1]))

    return Case("reverse_raster", "every unit exactly once, in reverse raster order", _with_state(one), reach,
                multi_mode=O.COLLAPSE, time_mode=O.DELTA_T, seed=203)


def _first_last_units():
    def one(case, rng):
        return steps_on(rng, np.where(rng.random(60) < 0.5, 0, case.n_units - 1), case.W, case.Cn)

    def reach(case):
        return all(set(np.unique(case.view(k)[0]).tolist()) == {0, case.n_units - 1} for k in (0, 2))

    return Case("first_last_units", "units 0 and n_units - 1 only", _with_state(one), reach, multi_mode=O.NORMAL,
                time_mode=O.DELTA_T, seed=204)


def _interleaved_hot():
    def one(case, rng):
        return steps_on(rng, np.tile(np.array([97, 640]), 200), case.W, case.Cn)

    def reach(case):
        ok = True
        for k in (0, 2):
            st = case.calls[k]
            keys = unit_keys(st, case.W, case.Cn, 0, case.rows)
            ok = ok and np.array_equal(keys, np.tile(np.array([97, 640], np.uint32), 200))
            # an unstable sort would be seen: neighbours inside a run differ
            _, order = case.view(k)
            run = st[order[:200]]
            ok = ok and np.count_nonzero(run[1:] != run[:-1]) > 150
        return ok

    return Case("interleaved_hot", "two hot units interleaved step by step: the sort's stability decides", _with_state(one),
                reach, multi_mode=O.COLLAPSE, time_mode=O.ABSOLUTE_T, seed=205)


# ---------------------------------------------------------------------------------------------------------------
# 4. channels and bands
# ---------------------------------------------------------------------------------------------------------------
def _channels():
    def build(case, rng):
        out = []
        for _ in range(3):
            st = case.rand(rng, 1200)
            st["c"] = rng.choice(np.array([0, 2, 0xFF, 1], np.uint8), len(st))
            out.append(st)
        return out

    def reach(case):
        ok = True
        for k in range(3):
            st = case.calls[k]
            keys, order = case.view(k)
            cs = st["c"][order]
            same_unit = keys[1:] == keys[:-1]
            # c = 0xFF lands on channel 0's unit, inside runs that also hold c = 0 steps
            mixed = np.any(same_unit & (cs[1:] != cs[:-1]))
            ok = ok and {0, 2, 0xFF} <= set(np.unique(st["c"]).tolist()) and bool(mixed) and keys[-1] != INVALID
        return ok

    return Case("channels_0_2_none", "3 channels with c = 0, 2 and 0xFF (channel 0)", build, reach, W=19, rows=7, Cn=3,
                multi_mode=O.NORMAL, time_mode=O.ABSOLUTE_T, crf=(0, 10), seed=301)


def _band(Cn, seed, mm, tm):
    def build(case, rng):
        out = []
        for _ in range(3):
            st = case.rand(rng, 1000)
            st["y"][:40] = np.where(rng.random(40) < 0.5, case.row_begin, case.row_begin + case.rows - 1)
            if Cn == 1:  # c = 0 names the one channel as well; the events carry the pixel's coordinate (no channel)
                st["c"][40:400] = 0
            out.append(st)
        return out

    def reach(case):
        ok = case.row_begin == 12 and case.rows == 5 and case.height == 23
        for k in range(3):
            y = case.calls[k]["y"]
            keys, _ = case.view(k)
            ok = ok and (Cn != 1 or set(np.unique(case.calls[k]["c"]).tolist()) == {0, 0xFF})
            ok = ok and y.min() == 12 and y.max() == 16 and keys[-1] != INVALID and keys[0] < case.W * case.Cn \
                and keys[-1] >= case.n_units - case.W * case.Cn
        return ok

    return Case(f"band_c{Cn}", f"rows 12..17 of 23, {Cn} channel(s): steps on the band's first and last row", build, reach,
                W=19, rows=5, Cn=Cn, row_begin=12, height=23, multi_mode=mm, time_mode=tm, seed=seed)


# ---------------------------------------------------------------------------------------------------------------
# 6. a quality change between calls
# ---------------------------------------------------------------------------------------------------------------
def _quality(mm, tm, band):
    def build(case, rng):
        return [case.rand(rng, 1500) for _ in range(6)]

    def reach(case):
        at, c_max, vel, dtm, base = case.quality_change
        return (at == 3 and len(case.calls) == 6 and (c_max, vel) != case.crf and dtm != case.delta_t_max
                and dtm % REF_TIME == 0 and all(_all_valid(case, k) for k in range(6)))

    geo = dict(W=19, rows=5, Cn=3, row_begin=12, height=23) if band else dict(W=37, rows=23, Cn=1)
    return Case(f"quality_mm{mm}_tm{tm}_{'band3' if band else 'gray'}",
                "set_crf_parameters + set_delta_t_max + reset_c_thresh between the third and fourth call", build, reach,
                multi_mode=mm, time_mode=tm, quality_change=(3, 3, 4, 1280, 1), seed=600 + 4 * mm + 2 * tm + band, **geo)


PARITY_CASES = (
    [_grid_case(n, i) for i, n in enumerate((1, 255, 256, 257, 1024, 1025))]
    + [_big_case(MERGE_SORT_LIMIT, "merge", 111, O.COLLAPSE, O.DELTA_T),
       _big_case(MERGE_SORT_LIMIT + 1, "onesweep", 112, O.NORMAL, O.ABSOLUTE_T)]
    + [_run_crosses_block(), _long_runs(), _reverse_raster(), _first_last_units(), _interleaved_hot()]
    + [_channels(), _band(3, 302, O.COLLAPSE, O.DELTA_T), _band(1, 303, O.NORMAL, O.ABSOLUTE_T)]
    + [_quality(mm, tm, band) for mm in (O.NORMAL, O.COLLAPSE) for tm in (O.DELTA_T, O.ABSOLUTE_T) for band in (0, 1)]
)


# ---------------------------------------------------------------------------------------------------------------
# 2. the workspace: sized at its first call, regrown when a call is larger, its temp storage sized for the capacity
# ---------------------------------------------------------------------------------------------------------------
def _workspace(name, sizes, seed, mm, tm):
    def build(case, rng):
        return [case.rand(rng, n, hot=0.05) for n in sizes]

    def reach(case):
        got = [len(c) for c in case.calls]
        cap, caps = 0, []
        for n in got:  # sparse_prepare
            if cap < n:
                cap = max(n, FIRST_WORKSPACE)
            caps.append(cap)
        paths = [sort_path(n) for n in got]
        if sizes[0] == 1:  # first allocation, exact fit, regrow by one, regrow to the onesweep size
            ok = caps == [4096, 4096, 4097, MERGE_SORT_LIMIT + 1]
        else:  # one workspace of 2^20 + 1 steps serves every smaller sort
            ok = caps == [MERGE_SORT_LIMIT + 1] * 5 and paths == ["onesweep", "merge", "merge", "block", "block"]
        return ok and got == list(sizes) and all(_all_valid(case, k) for k in range(len(got)))

    return Case(name, "workspace sizes " + " -> ".join(str(n) for n in sizes), build, reach, W=64, rows=32, multi_mode=mm,
                time_mode=tm, exact_cap=True, seed=seed)


WORKSPACE_CASES = [
    _workspace("workspace_growing", (1, 4096, 4097, MERGE_SORT_LIMIT + 1), 121, O.COLLAPSE, O.ABSOLUTE_T),
    _workspace("workspace_descending", (MERGE_SORT_LIMIT + 1, MERGE_SORT_LIMIT, 1025, 1024, 1), 122, O.NORMAL, O.DELTA_T),
]


# ---------------------------------------------------------------------------------------------------------------
# 5. refusals: lists with steps outside the band.  calls = [the refused list, a valid list for after reset()]
# ---------------------------------------------------------------------------------------------------------------
REFUSAL_KINDS = ("x_eq_width", "y_above_band", "y_eq_row_end", "c_eq_channels")
REFUSAL_PLACES = ("first", "last", "at_255", "at_256", "all")


def _spoil(case, st, kind, where):
    if kind == "x_eq_width":
        st["x"][where] = case.W
    elif kind == "y_above_band":
        st["y"][where] = case.row_begin - 1
    elif kind == "y_eq_row_end":
        st["y"][where] = case.row_begin + case.rows
    else:
        st["c"][where] = case.Cn


def _refusal(kind, place, seed):
    n = 600

    def build(case, rng):
        st = case.rand(rng, n)
        where = {"first": 0, "last": n - 1, "at_255": 255, "at_256": 256, "all": slice(None)}[place]
        _spoil(case, st, kind, where)
        return [st, case.rand(rng, 700)]

    def reach(case):
        keys = unit_keys(case.calls[0], case.W, case.Cn, case.row_begin, case.rows)
        bad = np.flatnonzero(keys == INVALID)
        want = {"first": [0], "last": [n - 1], "at_255": [255], "at_256": [256], "all": list(range(n))}[place]
        skeys, order = case.view(0)
        last = np.array_equal(np.sort(order[n - len(bad):]), bad) and np.all(skeys[: n - len(bad)] != INVALID)
        return bad.tolist() == want and bool(last) and _all_valid(case, 1)

    return Case(f"refuse_{kind}_{place}", f"a step with {kind}, placed {place}", build, reach, W=19, rows=5, Cn=3,
                row_begin=12, height=23, multi_mode=(O.NORMAL, O.COLLAPSE)[seed & 1],
                time_mode=(O.DELTA_T, O.ABSOLUTE_T)[(seed >> 1) & 1], seed=500 + seed)


REFUSAL_CASES = [_refusal(k, p, 5 * i + j) for i, k in enumerate(REFUSAL_KINDS) for j, p in enumerate(REFUSAL_PLACES)]


# ---------------------------------------------------------------------------------------------------------------
# 8. the depth boundary: hot pixels on an 8x4 plane.  P = the smallest max_depth at which the list passes (found with
# the sim, recorded here, checked by test_sparse_edges_cpu); overflow_at[d] = the first step that needs more than d
# nodes.  The unit of that step has at least three more steps in the same call: without the bound in cont_step the
# childless node such a step leaves behind reaches the root, the arena's length goes to 0, and the step after that
# indexes node 0xffffffff.
# ---------------------------------------------------------------------------------------------------------------
def _depth(name, seed, dtm, mm, tm, P, overflow_at):
    def build(case, rng):
        return [case.rand(rng, 4000)]

    def reach(case):
        keys = unit_keys(case.calls[0], case.W, case.Cn, 0, case.rows)
        ok = keys.max() != INVALID
        for d, i in overflow_at.items():
            ok = ok and d < P and np.count_nonzero(keys[i + 1:] == keys[i]) >= 3
        return bool(ok) and set(overflow_at) == {1, P - 1}

    c = Case(name, f"delta_t_max {dtm}: passes at max_depth {P}, not below", build, reach, W=8, rows=4, multi_mode=mm,
             time_mode=tm, delta_t_max=dtm, max_depth=P, start_frames=0, seed=seed)
    c.P, c.overflow_at = P, overflow_at
    return c


DEPTH_CASES = [
    _depth("depth_dtm160", 801, 160, O.NORMAL, O.DELTA_T, 9, {1: 1, 8: 802}),
    _depth("depth_dtm1280", 802, 1280, O.COLLAPSE, O.ABSOLUTE_T, 9, {1: 2, 8: 734}),
]

ALL_CASES = PARITY_CASES + WORKSPACE_CASES + REFUSAL_CASES + DEPTH_CASES


if __name__ == "__main__":  # `dump DIR`: the depth lists as raw AdderSparseStep records, for tools/sanitize/cont_step_depth.cpp
    import os
    import sys

    assert len(sys.argv) == 3 and sys.argv[1] == "dump", "usage: sparse_cases.py dump DIR"
    os.makedirs(sys.argv[2], exist_ok=True)
    args = []
    for case in DEPTH_CASES:
        path = os.path.join(sys.argv[2], case.name + ".steps")
        case.calls[0].tofile(path)
        args += [path, str(case.delta_t_max), str(int(case.multi_mode == O.COLLAPSE)), str(int(case.time_mode == O.ABSOLUTE_T)),
                 str(case.P)]
    with open(os.path.join(sys.argv[2], "args.txt"), "w") as f:
        f.write(" ".join(args) + "\n")
