"""Literal pure-Python restatement of the reference's adder-to-dvs (adder-to-dvs/src/main.rs:241-363, 450-460,
486-554) -- the yardstick of the ADDER -> DVS conversion (include/adder_dvs.h).  Times are Python ints (the
reference's u128), intensities go through math.log1p (the same libm log1p Rust's f64::ln_1p calls).

Errors follow the library's definition: the first event of a unit with d > 128, any event with d in 129..=254 and
any event outside the plane stop the run; run() returns the output of the events before it and the event's index.

DvsRestatement(.., census=c) also counts, per unit, the arms a run takes (tests/chain_arms.py names them); the output
does not depend on it.
"""
import math
import struct

D_ZERO_INTEGRATION, D_EMPTY = 128, 255
DELTA_T = 0


def is_framed(source_camera):
    return source_camera <= 5  # FramedU8 .. FramedF64 (adder-codec-core lib.rs:50-60)


def intensity_ln(d, t, ref):
    """event_to_frame_intensity (main.rs:450-460); d > 128 indexes D_SHIFT out of bounds there."""
    if d == D_ZERO_INTEGRATION:
        return 0.0
    if d > D_ZERO_INTEGRATION:
        raise IndexError(d)
    p = float(1 << d)
    if t == 0:
        return math.log1p((p * float(ref)) / 255.0)
    return math.log1p(((p / float(t)) * float(ref)) / 255.0)


class DvsRestatement:
    def __init__(self, width, height, channels, time_mode, ref_interval, source_camera, theta=0.01, census=None):
        self.w, self.h, self.ch = width, height, channels
        self.delta_t = time_mode == DELTA_T
        self.ref = ref_interval
        self.framed = is_framed(source_camera)
        self.theta = theta
        self.census = census
        self.px = {}  # (y, x, c) -> [d, frame_intensity_ln, t]

    @classmethod
    def from_meta(cls, meta, theta=0.01):
        return cls(meta["width"], meta["height"], meta["channels"], meta["time_mode"], meta["ref_interval"],
                   meta["source_camera"], theta)

    def run(self, events, units=None):
        """events: iterable of (x, y, c, d, t) (c 0xFF = None) or an EVENT_DTYPE array.  units: optional set of
        (y, x, c) to restrict the state to (units are independent).  -> (list of (t, x, y, p), bad index or None)."""
        out = []
        ref, theta, cen = self.ref, self.theta, self.census
        win_hi = math.log1p(1.0) - theta
        win_lo = math.log1p(0.0) + theta
        half = theta / 2.0
        for k, ev in enumerate(events):
            x, y, c, d, t = (int(v) for v in ((ev["x"], ev["y"], ev["c"], ev["d"], ev["t"]) if hasattr(ev, "dtype")
                                              else ev))
            c = 0 if c == 0xFF else c
            if not (x < self.w and y < self.h and c < self.ch):
                return out, k
            if D_ZERO_INTEGRATION < d < D_EMPTY:
                return out, k
            u = (y, x, c)
            if units is not None and u not in units:
                continue
            px = self.px.get(u)
            if px is None:
                if d > D_ZERO_INTEGRATION:
                    return out, k
                self.px[u] = [d, intensity_ln(d, t, ref), t]
                if cen is not None:
                    cen.hit("first", u)
                    cen.hit("d128" if d == D_ZERO_INTEGRATION else "t0" if t == 0 else "t_pos", u)
                continue
            old_t = px[2]
            if self.delta_t:
                px[2] += t
            else:
                px[2] = t
                if cen is not None and t < (old_t & 0xFFFFFFFF):
                    cen.hit("abs_saturate", u)
                t = max(0, t - (old_t & 0xFFFFFFFF))  # event.t.saturating_sub(old_t as u32)
            if self.framed and px[2] % ref != 0:
                px[2] = (px[2] // ref + 1) * ref
                if cen is not None:
                    cen.hit("rounded", u)
            if d == D_EMPTY:
                px[0] = d
                if cen is not None:
                    cen.hit("empty", u)
                continue
            new = intensity_ln(d, t, ref)
            old = px[1]
            win = 0.406 < new < 0.407
            if cen is not None:
                cen.hit("d128" if d == D_ZERO_INTEGRATION else "t0" if t == 0 else "t_pos", u)
                arm = _arm(win, new, old, px[2] == old_t, win_hi, win_lo, half)
                cen.hit(arm, u)
            if win and (old > win_hi or (px[2] == old_t and old > 0.6)):
                p = 1
            elif win and (old < win_lo or (px[2] == old_t and old < 0.3)):
                p = 0
            elif new > old + half:
                p = 1
            elif new < old - half:
                p = 0
            else:
                p = None
            assert cen is None or _ARM_POLARITY[arm] == p
            if p is not None:
                out.append((old_t + 1, x, y, p))
                px[1] = new
            px[0] = d
        return out, None


_ARM_POLARITY = dict(win_hi=1, win_same_hi=1, win_lo=0, win_same_lo=0, up=1, down=0, none=None)


def _arm(win, new, old, same_t, win_hi, win_lo, half):
    """census only: the name of the arm the four-way test of run() takes"""
    if win and old > win_hi:
        return "win_hi"
    if win and same_t and old > 0.6:
        return "win_same_hi"
    if win and old < win_lo:
        return "win_lo"
    if win and same_t and old < 0.3:
        return "win_same_lo"
    return "up" if new > old + half else "down" if new < old - half else "none"


def header_bytes(width, height, date, binary):
    h = f"% Height {height}\n% Width {width}\n% Version 2\n% Date {date}\n% end\n".encode()
    return h + (b"\x00\x08" if binary else b"")


def dat_bytes(out):
    return b"".join(struct.pack("<II", t & 0xFFFFFFFF, (p << 28) | (y << 14) | x) for t, x, y, p in out)


def text_bytes(out):
    return "".join(f"{t} {x} {y} {p}\n" for t, x, y, p in out).encode()


def reorder(out):
    """Our definition of --reorder: a stable sort by the 32-bit t."""
    return sorted(out, key=lambda e: e[0] & 0xFFFFFFFF)


def file_bytes(meta, out, date, text=False, reorder_=False, bad=None):
    """What the reference writes for a run: header, then the records.  With --reorder the queue is written only
    when the run ends without an error (main.rs:373-377 follows the loop; an error returns before it)."""
    hdr = header_bytes(meta["width"], meta["height"], date, not text)
    if text:
        return hdr + text_bytes(out)
    if reorder_:
        return hdr + (b"" if bad is not None else dat_bytes(reorder(out)))
    return hdr + dat_bytes(out)
