"""Literal pure-Python restatement of the reference's stream migration (adder-codec-rs/src/utils/stream_migration.rs:
32-88, src/bin/migrate_raw_v0_v1_to_v2.rs), of its inverse as include/adder_stream.h defines it, and of adder-info
(adder-info/src/main.rs:30-153) -- the yardstick of include/adder_stream.h.  Times are Python ints (the reference's
u32, with our overflow errors), intensities Python floats (f64).

Errors follow the library's definition: forward, T + t above u32::MAX; inverse and AbsoluteT info, t below the unit's
previous time; any event outside the plane.  A run returns what the events before the bad one give, and its index.
"""
import math
import struct

D_ZERO_INTEGRATION, D_EMPTY = 128, 255
DELTA_T, ABSOLUTE_T, MIXED = 0, 1, 2
U32_MAX = (1 << 32) - 1
F64_MAX = 1.7976931348623157e308
CAMERAS = ["FramedU8", "FramedU16", "FramedU32", "FramedU64", "FramedF32", "FramedF64", "Dvs", "DavisU8", "Atis",
           "Asint"]
TIME_MODES = ["DeltaT", "AbsoluteT", "Mixed"]
EOF = bytes([0xFF, 0xFF, 0xFF, 0xFF, 0x01, 0, 0, 0, 0, 0, 0])


def is_framed(source_camera):
    return source_camera <= 5  # FramedU8 .. FramedF64 (adder-codec-core lib.rs:50-60)


def _fields(ev):
    x, y, c, d, t = (int(v) for v in ((ev["x"], ev["y"], ev["c"], ev["d"], ev["t"]) if hasattr(ev, "dtype") else ev))
    return x, y, c, (0 if c == 0xFF else c), d, t


def in_time_mode(meta):
    return meta["time_mode"] if meta["version"] >= 2 else DELTA_T  # a v0 / v1 header has no time-mode field


class Migration:
    """meta: width, height, channels, version, time_mode, ref_interval, source_camera (the INPUT stream's)."""

    def __init__(self, meta, out_time_mode):
        self.meta, self.out = meta, out_time_mode
        self.t = {}  # (y, x, c) -> the unit's time
        src = in_time_mode(meta)
        self.direction = ("forward" if (src, out_time_mode) == (DELTA_T, ABSOLUTE_T) else
                          "inverse" if (src, out_time_mode) == (ABSOLUTE_T, DELTA_T) else "pass")

    def run(self, events):
        """-> (list of (x, y, c, d, t) with c as it came in, bad index or None)"""
        m = self.meta
        ref, framed = m["ref_interval"], is_framed(m["source_camera"])
        out = []
        for k, ev in enumerate(events):
            x, y, c_raw, c, d, t = _fields(ev)
            if not (x < m["width"] and y < m["height"] and c < m["channels"]):
                return out, k
            u = (y, x, c)
            if self.direction == "forward":  # migrate_v2
                T = self.t.get(u, 0) + t
                if T > U32_MAX:
                    return out, k
                t = T
                if m["version"] > 0 and framed and T % ref > 0:
                    T = (T // ref + 1) * ref
                self.t[u] = T
            elif self.direction == "inverse":
                L = self.t.get(u, 0)
                if t < L:
                    return out, k
                L, t = t, t - L
                if framed and L % ref != 0:
                    L = (L // ref + 1) * ref
                self.t[u] = L
            out.append((x, y, c_raw, d, t))
        return out, None


def migrated_header(header, time_mode):
    """The input's header with time_mode set and the codec version raised to 2 where it was below."""
    version = header[5]
    cam = struct.unpack(">I", header[25:29])[0] if version >= 1 else 0
    out = bytearray(header[:25]) + struct.pack(">II", cam, time_mode)
    out[5] = max(version, 2)
    if version >= 3:
        out += header[33:37]
    return bytes(out)


def event_to_intensity(d, t):
    """scale_intensity.rs:262-270; D_SHIFT_F64[128] is 0"""
    if d > D_ZERO_INTEGRATION:
        return 0.0
    p = 0.0 if d == D_ZERO_INTEGRATION else float(1 << d)
    return p if t == 0 else p / float(t)


FOLD_ARMS = ("ignored", "lower", "replace_by_128", "replace_by_inf", "to_zero", "sticky", "offered_and_raises",
             "offered_and_does_not")


class Info:
    """census: an optional list; run() appends the arm (one of FOLD_ARMS) that each folded event took.  ignored:
    D_EMPTY; lower: a < min, min = a; replace_by_128 / replace_by_inf: d == 128 sets min = 1 / t (t > 0 / t == 0);
    to_zero: d in 129..=254 sets min = 0.0; sticky: d >= 128 met min == 0.0 and moved nothing; offered_and_raises /
    offered_and_does_not: a >= min, offered to max."""

    def __init__(self, meta, census=None):
        self.meta, self.census = meta, census
        self.absolute = meta["version"] >= 2 and meta["time_mode"] == ABSOLUTE_T
        self.last_t = {}
        self.min, self.max, self.count = F64_MAX, 0.0, 0

    def run(self, events):
        """folds the events (main.rs:90-121); -> bad index or None"""
        m = self.meta
        for k, ev in enumerate(events):
            x, y, _, c, d, t = _fields(ev)
            if not (x < m["width"] and y < m["height"] and c < m["channels"]):
                return k
            if self.absolute:
                u = (y, x, c)
                last = self.last_t.get(u, 0)
                if t < last:
                    return k
                self.last_t[u] = t
                t -= last
            a = event_to_intensity(d, t)
            if d == D_EMPTY:
                arm = "ignored"
            elif math.isinf(a):
                arm = None  # unreachable: no intensity is infinite
            elif a < self.min:
                if d == D_ZERO_INTEGRATION:
                    self.min = 1.0 / t if t != 0 else math.inf
                    arm = "replace_by_128" if t != 0 else "replace_by_inf"
                else:
                    self.min = a
                    arm = "to_zero" if d > D_ZERO_INTEGRATION else "lower"
            elif a > self.max:
                self.max = a
                arm = "offered_and_raises"
            else:
                arm = "sticky" if d >= D_ZERO_INTEGRATION else "offered_and_does_not"
            if self.census is not None:
                self.census.append(arm)
            self.count += 1
        return None


def rust_f4(x):
    """Rust's {:.4}"""
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "-inf" if x < 0 else "inf"
    return "%.4f" % x


def _log(fn, x):
    if math.isnan(x):
        return math.nan
    if x == 0.0:
        return -math.inf
    if x < 0.0:
        return math.nan
    return math.inf if math.isinf(x) else fn(x)


def _div(a, b):
    """IEEE division of non-negative doubles"""
    if math.isnan(a) or math.isnan(b):
        return math.nan
    if b == 0.0:
        return math.nan if a == 0.0 else math.inf
    if math.isinf(a):
        return math.nan if math.isinf(b) else math.inf
    return a / b


def report(meta, header_size, file_size, n_events, dynamic_range=False, min_intensity=F64_MAX, max_intensity=0.0):
    """The report's text (main.rs:47-66, 137-147) with the event count given and without the progress line."""
    volume = meta["width"] * meta["height"] * meta["channels"]
    lines = ["Dimensions", f"\tWidth: {meta['width']}", f"\tHeight: {meta['height']}",
             f"\tColor channels: {meta['channels']}", f"Source camera: {CAMERAS[meta['source_camera']]}",
             "ADΔER transcoder parameters", f"\tCodec version: {meta['version']}",
             # decoder.rs:119-123, 178: without a v2 extension the metadata keeps TimeMode::default() = AbsoluteT
             f"\tTime mode: {TIME_MODES[meta['time_mode'] if meta['version'] >= 2 else ABSOLUTE_T]}",
             f"\tTicks per second: {meta['tps']}",
             f"\tReference ticks per source interval: {meta['ref_interval']}", f"\tΔt_max: {meta['delta_t_max']}",
             "File metadata", f"\tFile size: {file_size}", f"\tHeader size: {header_size}",
             f"\tADΔER event count: {n_events}", f"\tEvents per pixel channel: {n_events // volume}"]
    if dynamic_range:
        theory = _div(0.0, _div(1.0, float(meta["delta_t_max"])))  # D_SHIFT[128] as f64 / (1 / delta_t_max)
        real = _div(max_intensity, min_intensity)
        lines += ["Dynamic range", "\tTheoretical range:", f"\t\t{rust_f4(10.0 * _log(math.log10, theory))} dB (power)",
                  f"\t\t{rust_f4(_log(math.log2, theory))} bits", "\tRealized range:",
                  f"\t\t{rust_f4(10.0 * _log(math.log10, real))} dB (power)",
                  f"\t\t{rust_f4(_log(math.log2, real))} bits"]
    return "\n".join(lines) + "\n"
