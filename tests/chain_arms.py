"""An arm census of the two chain oracles (tests/prophesee_oracle.py, tests/dvs_oracle.py): how often, and on how many
different pixels, a run takes each branch of the per-pixel walk that pph_walk_kernel / pph_end_kernel and
dvs_ln_kernel / dvs_walk_kernel restate.  The oracles fill a Census only when they are given one.

Prophesee arms: skip (t < lt), same_t (t == lt), step_no_gap (t == lt + 1), gap, gap_clamp_hi / gap_clamp_lo,
step_clamp_hi / step_clamp_lo, gap_time_wrap (gap * ref_time >= 2^32), t_over_2p24 / t_over_2p31 (a step whose time,
or a pixel whose f32 running time, is above 2^24 / 2^31), end_span_wrap (end_events: d * ref_time >= 2^32).
DVS arms: first, empty, d128, t0, rounded, abs_saturate, win_hi, win_same_hi, win_lo, win_same_lo, up, down, none.
"""
from collections import Counter, defaultdict

PROPHESEE_ARMS = ("skip", "same_t", "step_no_gap", "gap", "gap_clamp_hi", "gap_clamp_lo", "step_clamp_hi",
                  "step_clamp_lo", "gap_time_wrap", "t_over_2p24", "t_over_2p31", "end_span_wrap")
DVS_ARMS = ("first", "empty", "d128", "t0", "rounded", "abs_saturate", "win_hi", "win_same_hi", "win_lo",
            "win_same_lo", "up", "down", "none")
SINGLE = ("gap_time_wrap", "end_span_wrap")  # arms that one occurrence covers


class Census:
    def __init__(self):
        self.count = Counter()
        self.pixels = defaultdict(set)

    def hit(self, arm, pixel):
        self.count[arm] += 1
        self.pixels[arm].add(pixel)

    def reached(self, arm):
        """The condition a constructed case must meet for an arm it is meant to reach: 4 times on 2 pixels."""
        if arm in SINGLE:
            return self.count[arm] >= 1
        return self.count[arm] >= 4 and len(self.pixels[arm]) >= 2

    def missing(self, arms):
        return [(a, self.count[a], len(self.pixels[a])) for a in arms if not self.reached(a)]


def prophesee_census(recs, W, H, ref_time, crf=None):
    """recs: RECORD_DTYPE array or .dat body bytes -> (Census, the oracle after the run, its events)."""
    import prophesee_oracle as R
    c = Census()
    src = R.Prophesee(W, H, ref_time, crf, census=c)
    ev = src.run(R.decode_body(recs.tobytes() if hasattr(recs, "tobytes") else recs))
    return c, src, ev


def dvs_census(meta, events, theta=0.01):
    """-> (Census, the restatement's output, bad index or None)."""
    import dvs_oracle as R
    c = Census()
    r = R.DvsRestatement(meta["width"], meta["height"], meta["channels"], meta["time_mode"], meta["ref_interval"],
                         meta["source_camera"], theta, census=c)
    out, bad = r.run(events)
    return c, out, bad
