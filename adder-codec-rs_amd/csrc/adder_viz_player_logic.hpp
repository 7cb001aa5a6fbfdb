// adder_viz_player_logic.hpp -- the pop schedule of the adder-viz player (include/adder_viz_player.h), shared by the
// schedule kernel (one workgroup, rows spread over its threads) and the host (adder_viz_schedule_host, rows in a loop).
//
// What a call knows when the schedule runs (indices are LOCAL to the call, -1 = "before the call's first event"):
//   cnt_carry[r][slot]  fills of (row r, pending frame) by earlier calls that were in time; slot = frame % ring
//   cnt_call / nat_call the same for this call's fills, with the largest event index among them (-1: none).  A fill of
//                       a frame the call pops may be late; such a frame is never looked at again once it is popped,
//                       and a frame that is complete in time has no late fills (a unit fills a frame once).
//   comb[p]             the call's checked events ordered by row (stable, so in stream order inside a row), as the
//                       inclusive maximum of (row << 32 | L + 1): inside a row the low word is the row's prefix
//                       maximum of L, and the whole array ascends, so "the first event of row r with L > thr" is one
//                       binary search.  It needs no lower bound s: when a period opens, every earlier event has
//                       L <= W + limit - 1 (the pops before it ran until max(M, W) - W + 1 <= limit), so none forces.
//   pm[i]               inclusive prefix maximum of L in input order (gives M at any E)
//   done_carry[r]       the row's chunk_filled_tracker entry as the last call left it; it holds for the period that
//                       was open then, i.e. until the call's first pop
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ADDER_VIZ_HD __host__ __device__ __forceinline__
#else
#define ADDER_VIZ_HD inline
#endif

namespace adder {

constexpr int64_t kVizInf = (int64_t)1 << 62;  // +inf of event indices

struct VizSchedIn {
    int64_t n;      // the call's events that count (those before a bad event / the end of the wire stream)
    int64_t n_all;  // the call's records: the length of the row order (those past n carry L = -1 and never force)
    const unsigned long long *comb;  // n_all
    const uint32_t *ridx;            // n_all: input index of row-ordered position p
    const int32_t *pm;               // n
    const uint32_t *cnt_carry, *cnt_call;  // rows * ring
    const int32_t *nat_call;               // rows * ring
    const uint8_t *done_carry;             // rows
    uint32_t rows, row_units, ring;
    int32_t w0;  // frames_written before the call
    int32_t m0;  // largest L of any earlier event (-1: none)
    int32_t has_limit;
    uint32_t limit;
    int32_t opening;  // the limit was set since the last call: the loop in front of the read loop runs first
    int32_t finish;
    uint32_t max_pops;  // room of pops / flushed
};

struct VizSchedOut {
    int32_t *pops;     // local index of the event after which frame w0 + k is popped
    uint8_t *flushed;  // finish filled the frame's Nones
    uint8_t *done;     // rows: the tracker for the period left open
    uint32_t n_pops;
    uint32_t overflow;  // more than max_pops
    int32_t w_end, m_end;
};

// nat_r(f): -1 (= -inf: complete by earlier calls alone), a local event index, or kVizInf
ADDER_VIZ_HD int64_t viz_nat(const VizSchedIn &v, uint32_t r, int64_t f) {
    if (f < (int64_t)v.w0 || f >= (int64_t)v.w0 + (int64_t)v.ring) return kVizInf;  // nothing is kept for it
    const size_t at = (size_t)r * v.ring + (size_t)(f % (int64_t)v.ring);
    if (v.cnt_carry[at] + v.cnt_call[at] < v.row_units) return kVizInf;
    return (int64_t)v.nat_call[at];
}

// forced_r(W): the first checked event of row r in this call with L > W + limit
ADDER_VIZ_HD int64_t viz_forced(const VizSchedIn &v, uint32_t r, int64_t w) {
    if (!v.has_limit) return kVizInf;
    const int64_t low = w + (int64_t)v.limit + 1;  // L + 1 > low
    if (low >= (int64_t)0xffffffffll) return kVizInf;
    const unsigned long long key = ((unsigned long long)r << 32) | (unsigned long long)low;
    int64_t lo = 0, hi = v.n_all;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (v.comb[mid] > key)
            hi = mid;
        else
            lo = mid + 1;
    }
    if (lo >= v.n_all || (uint32_t)(v.comb[lo] >> 32) != r) return kVizInf;
    return (int64_t)v.ridx[lo];
}

ADDER_VIZ_HD int64_t viz_min(int64_t a, int64_t b) { return a < b ? a : b; }
ADDER_VIZ_HD int64_t viz_max(int64_t a, int64_t b) { return a > b ? a : b; }

// the `chunk.len() > buffer_limit` clause: a row's deque holds max(maxL_r, W) - W + 1 frames
ADDER_VIZ_HD bool viz_over_limit(const VizSchedIn &v, int64_t m, int64_t w) {
    return v.has_limit && viz_max(m, w) - w + 1 > (int64_t)v.limit;
}

// `red.max_rows(fn)` = max over rows of fn(r), the same value in every thread; `red.leader()` = the thread that
// writes.  Every thread runs the same control flow (all branches depend on reduced values only).
template <class Red>
ADDER_VIZ_HD void viz_schedule(const VizSchedIn &v, Red &red, VizSchedOut &o) {
    int64_t w = v.w0;
    uint32_t np = 0;
    bool overflow = false;
    auto m_at = [&](int64_t e) -> int64_t { return e < 0 ? (int64_t)v.m0 : viz_max((int64_t)v.m0, (int64_t)v.pm[e]); };
    auto pop = [&](int64_t e, uint8_t flushed) {
        if (np >= v.max_pops) {
            overflow = true;
            return;
        }
        if (red.leader()) {
            o.pops[np] = (int32_t)e;
            o.flushed[np] = flushed;
        }
        ++np;
        ++w;
    };
    // `while is_frame_0_filled()` right after event e (adder.rs:339): the trackers are the carried ones until the
    // call's first pop, a pop recomputes them from the frame's own count
    auto cascade = [&](int64_t e) {
        const int64_t m = m_at(e);
        while (!overflow) {
            bool go = viz_over_limit(v, m, w);
            if (!go) {
                const bool carried = np == 0u;
                const int64_t c = red.max_rows([&](uint32_t r) -> int64_t {
                    if (carried) return v.done_carry[r] ? (int64_t)-1 : kVizInf;
                    return viz_nat(v, r, w);
                });
                go = c <= e;
            }
            if (!go) break;
            pop(e, 0u);
        }
    };
    if (v.opening) cascade(-1);
    while (!overflow) {
        const bool carried = np == 0u;
        const int64_t e = red.max_rows([&](uint32_t r) -> int64_t {
            if (carried && v.done_carry[r]) return (int64_t)-1;
            return viz_min(viz_nat(v, r, w), viz_forced(v, r, w));
        });
        if (e >= kVizInf) break;  // the period stays open
        pop(e, 0u);
        cascade(e);
    }
    if (v.finish) {  // the Err arm: flush_frame_buffer while some deque holds more than one frame
        const int64_t m = m_at(v.n - 1);
        while (!overflow && m > w) {
            pop(v.n - 1, 1u);
            cascade(v.n - 1);
        }
    }
    // the trackers of the period left open
    const bool carried = np == 0u;
    red.for_rows([&](uint32_t r) {
        o.done[r] = ((carried && v.done_carry[r]) || viz_nat(v, r, w) < kVizInf || viz_forced(v, r, w) < kVizInf) ? 1u : 0u;
    });
    if (red.leader()) {
        o.n_pops = np;
        o.overflow = overflow ? 1u : 0u;
        o.w_end = (int32_t)w;
        o.m_end = (int32_t)m_at(v.n - 1);
    }
}

// rows in a loop: the host's reducer
struct VizSerialRows {
    uint32_t rows;
    ADDER_VIZ_HD bool leader() const { return true; }
    template <class F>
    ADDER_VIZ_HD int64_t max_rows(F f) const {
        int64_t m = -kVizInf;
        for (uint32_t r = 0; r < rows; ++r) m = viz_max(m, f(r));
        return m;
    }
    template <class F>
    ADDER_VIZ_HD void for_rows(F f) const {
        for (uint32_t r = 0; r < rows; ++r) f(r);
    }
};

}  // namespace adder
