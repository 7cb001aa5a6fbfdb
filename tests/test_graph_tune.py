"""The graph tuner's decisions (adder-codec-rs_amd/csrc/adder_graph_tune.hpp): which instance of a captured batch runs
next, who is chosen, who is retired, which key leaves a full cache -- driven on the CPU.  The header is the one
libadder_hip.so compiles (adder_hip_graphs.cpp); g++ builds it here with a small C shim (tests/cpu_sim/graph_tune.cpp).
The expectations are the schedule as it stood inside get_graph / graph_tune_report."""
import ctypes as C
import os
import subprocess

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_CSRC = os.path.join(_ROOT, "adder-codec-rs_amd", "csrc")
_SRC = os.path.join(_HERE, "cpu_sim", "graph_tune.cpp")
_LIB = os.path.join(_HERE, "cpu_sim", "libadder_graph_tune.so")
_DEPS = [_SRC, os.path.join(_CSRC, "adder_graph_tune.hpp"), os.path.join(_CSRC, "adder_variant.hpp")]

COLLAPSE, GENERIC = 1, 4
CACHE_KEYS = 24
NEVER = 1e30  # a candidate's best time before a run of it has counted

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(p) for p in _DEPS):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                                   "-I", _CSRC, "-I", os.path.join(_ROOT, "include"), _SRC, "-o", _LIB])
        L = C.CDLL(_LIB)
        L.tune_new.restype = C.c_void_p
        L.tune_delete.argtypes = [C.c_void_p]
        L.tune_pick_c.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_size_t),
                                  C.POINTER(C.c_int)]
        L.tune_add_c.argtypes = [C.c_void_p, C.c_uint64, C.c_size_t]
        L.tune_report_c.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
        L.tune_retire_all_c.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
        for f in (L.tune_settled_c, L.tune_pending_c, L.tune_keys_c):
            f.argtypes = [C.c_void_p]
        L.tune_best_ms_c.restype = C.c_float
        L.tune_best_ms_c.argtypes = [C.c_void_p, C.c_uint64, C.c_int]
        L.tune_graph_candidates.restype = C.c_uint32
        L.tune_graph_candidates.argtypes = [C.c_uint32] * 4
        _lib = L
    return _lib


class Cache:
    """A GraphCache with made-up handles: key k's n-th instance is 1000 * k + n + 1."""

    def __init__(self):
        self.L = lib()
        self.gc = self.L.tune_new()
        self.made = {}          # key -> instances made so far
        self.one_stream = {}    # handle -> the kind tune_pick asked for
        self.retired = []       # every handle handed back, in order

    def close(self):
        self.L.tune_delete(self.gc)

    def _drain(self, buf, n):
        self.retired += [buf[i] for i in range(n.value)]

    def pick(self, key, want):
        """tune_pick; returns (candidate or -1, one_stream)"""
        buf, n, one = (C.c_size_t * 64)(), C.c_int(0), C.c_int(0)
        use = self.L.tune_pick_c(self.gc, key, want, C.byref(one), buf, C.byref(n))
        self._drain(buf, n)
        return use, bool(one.value)

    def batch(self, key, want):
        """What get_graph does for one batch: the candidate that runs it, instantiated first when the tuner asks."""
        use, one = self.pick(key, want)
        if use < 0:
            h = 1000 * key + self.made.get(key, 0) + 1
            self.made[key] = self.made.get(key, 0) + 1
            self.one_stream[h] = one
            use = self.L.tune_add_c(self.gc, key, h)
        return use

    def report(self, ms):
        """tune_report; returns the chosen candidate when this report settled the choice, else -1"""
        buf, n = (C.c_size_t * 64)(), C.c_int(0)
        chosen = self.L.tune_report_c(self.gc, ms, buf, C.byref(n))
        self._drain(buf, n)
        return chosen

    def best(self, key, cand):
        return self.L.tune_best_ms_c(self.gc, key, cand)

    def settled(self):
        return bool(self.L.tune_settled_c(self.gc))

    def pending(self):
        return bool(self.L.tune_pending_c(self.gc))

    def keys(self):
        return self.L.tune_keys_c(self.gc)


@pytest.fixture
def cache():
    c = Cache()
    yield c
    c.close()


def tune(c, key, want, ms_of):
    """Runs batches of `key` until the choice; ms_of(candidate, its run number from 1) is each batch's time.
    Returns (the candidates in the order they ran, the chosen one)."""
    order, runs = [], {}
    for _ in range(4 * want + 8):
        use = c.batch(key, want)
        order.append(use)
        runs[use] = runs.get(use, 0) + 1
        chosen = c.report(ms_of(use, runs[use]))
        if chosen >= 0:
            return order, chosen
        assert not c.settled()
    raise AssertionError("no choice after %d batches: %r" % (len(order), order))


@pytest.mark.parametrize("want", [2, 3, 6])
def test_schedule(cache, want):
    """Candidate 0 twice, 1 twice, ..., want-1 twice, then candidate 0 twice more; 2 * want + 2 batches before the
    choice; the first instance is the one-stream one, every later one two-branch."""
    order, chosen = tune(cache, 7, want, lambda k, run: 1.0)
    assert order == [k for k in range(want) for _ in (0, 1)] + [0, 0]
    assert len(order) == 2 * want + 2
    assert chosen == 0  # (equal times: the one-stream instance keeps the batch)
    assert [cache.one_stream[7000 + n + 1] for n in range(want)] == [True] + [False] * (want - 1)
    assert sorted(cache.retired) == [7000 + n + 1 for n in range(1, want)]
    assert cache.settled() and not cache.pending()
    # settled: the chosen one runs every later batch, nothing is instantiated, no time is wanted
    assert cache.pick(7, want)[0] == 0 and not cache.pending()
    assert cache.made[7] == want


def test_one_candidate_settles_after_two_batches(cache):
    order, chosen = tune(cache, 3, 1, lambda k, run: 2.0)
    assert order == [0, 0] and chosen == 0
    assert cache.retired == [] and cache.one_stream[3001] is True


def test_first_run_never_counts(cache):
    """A candidate's first run also uploads the instance: however fast it looks, it is not its best time."""
    for cand, second in ((0, 1.02), (1, 1.12)):
        assert cache.batch(9, 3) == cand
        assert cache.report(0.001) == -1
        assert cache.best(9, cand) == pytest.approx(NEVER)
        assert cache.batch(9, 3) == cand
        assert cache.report(second) == -1
        assert cache.best(9, cand) == pytest.approx(second)


@pytest.mark.parametrize("times, expect", [
    ([1.0, 0.99], 0),            # a two-branch instance must beat the one-stream one by the factor 0.985
    ([1.0, 0.986], 0),
    ([1.0, 0.98], 1),
    ([1.0, 0.98, 0.975], 2),     # ... and, once one has, a later one only has to beat that one
    ([1.0, 0.98, 0.98], 1),
    ([1.0, 0.99, 0.986], 0),
    ([1.0, 1.2, 0.5, 0.9], 2),
])
def test_choice(cache, times, expect):
    want = len(times)
    order, chosen = tune(cache, 11, want, lambda k, run: 0.001 if run == 1 else times[k])
    assert chosen == expect
    assert sorted(cache.retired) == [11000 + n + 1 for n in range(want) if n != expect]


def test_recheck_runs_count_for_candidate_0(cache):
    """Candidate 0 ran first, on a cold chip: its two extra runs after the others count toward its best time."""
    # candidate 0: 1.0 when it was new, 0.9 in the recheck; candidate 1: 0.89 -- beats 1.0 * 0.985, not 0.9 * 0.985
    order, chosen = tune(cache, 13, 2, lambda k, run: [None, 0.001, 1.0, 0.9, 0.95][run] if k == 0 else 0.89)
    assert order == [0, 0, 1, 1, 0, 0]
    assert chosen == 0
    assert cache.best(13, 0) == pytest.approx(0.9)


def test_report_without_pending_batch_changes_nothing(cache):
    assert cache.report(1.0) == -1  # nothing was ever queued
    cache.batch(5, 2)
    assert cache.pending()
    assert cache.report(1.0) == -1 and not cache.pending()
    assert cache.report(0.5) == -1  # a second report for the same batch
    assert cache.batch(5, 2) == 0   # (the first report counted as run 1: candidate 0 has its second run now)
    cache.report(1.0)
    assert cache.best(5, 0) == pytest.approx(1.0)
    assert cache.retired == []


def test_report_for_an_evicted_key_changes_nothing(cache):
    cache.batch(1, 2)  # key 1's batch is in flight
    for key in range(2, 2 + CACHE_KEYS):  # 24 more keys are asked for (their instantiation "fails": nothing is added)
        assert cache.pick(key, 2)[0] == -1
    assert cache.keys() == CACHE_KEYS
    assert cache.retired == [1001]  # key 1, the smallest, went when the 25th key came
    assert cache.report(1.0) == -1
    assert cache.keys() == CACHE_KEYS and cache.retired == [1001]
    assert cache.best(1, 0) == -1.0


def test_full_cache_evicts_the_smallest_key_with_all_its_live_candidates(cache):
    # key 2, still choosing: two live candidates
    for _ in range(3):
        cache.batch(2, 3)
        cache.report(1.0)
    assert cache.made[2] == 2
    # key 4, settled on candidate 1: candidate 0 was retired at the choice
    tune(cache, 4, 2, lambda k, run: 1.0 if k == 0 else 0.5)
    assert cache.retired == [4001]
    for key in range(10, 10 + CACHE_KEYS - 2):
        cache.batch(key, 1)
        cache.report(1.0)
    assert cache.keys() == CACHE_KEYS and cache.retired == [4001]
    cache.batch(100, 1)  # the 25th key
    assert cache.keys() == CACHE_KEYS
    assert cache.retired == [4001, 2001, 2002]
    assert cache.best(2, 0) == -1.0 and cache.best(4, 1) == pytest.approx(0.5)
    cache.report(1.0)
    cache.batch(101, 1)  # the next one takes key 4: only its chosen instance is left to hand back
    assert cache.retired == [4001, 2001, 2002, 4002]
    # a key that comes back starts over
    assert cache.pick(2, 3) == (-1, True)


def test_retire_all(cache):
    tune(cache, 4, 2, lambda k, run: 1.0 if k == 0 else 0.5)
    cache.batch(6, 2)
    buf = (C.c_size_t * 64)()
    n = cache.L.tune_retire_all_c(cache.gc, buf)
    assert sorted(buf[i] for i in range(n)) == [4002, 6001]
    assert cache.keys() == 0 and not cache.pending() and cache.settled()


def test_graph_candidates():
    """variant_graph_candidates decides `want`: several candidates only for a lean batch longer than a chunk."""
    L = lib()
    assert L.tune_graph_candidates(COLLAPSE, 300, 64, 6) == 6
    assert L.tune_graph_candidates(COLLAPSE, 65, 64, 3) == 3
    assert L.tune_graph_candidates(COLLAPSE, 64, 64, 6) == 1   # one chunk: nothing to overlap
    assert L.tune_graph_candidates(COLLAPSE | GENERIC, 300, 64, 6) == 1  # captured on one stream anyway
    assert L.tune_graph_candidates(COLLAPSE, 300, 64, 1) == 1
