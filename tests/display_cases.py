"""Inputs for the edge tests of the display frame (adder_display.hip): planes more than one tile wide, clips that put
feature crosses on every tile boundary, and the clips of the rollback / reset tests.  No GPU here: test_display_cases_cpu.py
shows on the CPU oracle alone that the inputs reach what they are built for, test_gpu_display_edges.py runs them.

Shapes come from the kernel's named constants (kernel_constants.display()), so they move with a retune: T bytes of a row
and R rows per workgroup.  The expected frame is oracle.Video's plane with live_view_oracle.draw_crosses on its
feature_set() (Hold) or new_features() (Instant) -- what live_view_oracle.LiveView._handle_features does, without its
per-pixel Python loop."""
import functools

import numpy as np

import kernel_constants
import live_view_oracle as R
from oracle import oracle as O

K = kernel_constants.display()
T = K["kDisplayTileBytes"]   # bytes of a row one workgroup covers
ROWS = K["kDisplayRows"]     # rows one workgroup covers
CROSS_REACH = 2              # draw_feature_coord: -2 ..= 2 (adder_pixel.hpp kCrossReach; utils/viz.rs:94-120)
FAST_BORDER = 3              # the corner test's circle: centres lie 3 pixels inside the plane

H = 13                       # row tiles 0-3, 4-7, 8-11, 12 (R = 4); FAST admits centres on rows 3 .. 9
FRAMES = 7
DTM = 7650
MAX_DEPTH = 30


def check_constants():
    """The shapes below assume whole pixels (1 and 3 channels) and whole 16-byte lines per tile."""
    assert T % 48 == 0, f"kDisplayTileBytes = {T} is no multiple of 48: a tile no longer holds whole RGB pixels and whole " \
                        "16-byte lines, and the planes of display_cases.py no longer end where they say"
    assert FAST_BORDER <= ROWS - 1 and ROWS - 1 + 6 <= H - 1 - FAST_BORDER, \
        f"kDisplayRows = {ROWS}: the centres' rows R-1 .. R+5 leave the rows FAST admits ({FAST_BORDER} .. {H - 1 - FAST_BORDER})"


check_constants()

# (W, H, Cn): row lengths T+5 (a last tile of 5 bytes: byte-wise stores only), 2T+40 (a full middle tile), and in RGB
# T+12 (a last tile 4 pixels wide) and 2T+84
PLANES = ((T + 5, H, 1), (2 * T + 40, H, 1), (T // 3 + 4, H, 3), (2 * T // 3 + 28, H, 3))
PLANE_IDS = ["%dx%dx%d" % p for p in PLANES]
SMALL_PLANES = ((70, 37, 1), (33, 19, 3))   # test_gpu_live_view.py's: one tile in x


def tiles_per_row(W, Cn):
    return (W * Cn + T - 1) // T


def boundaries(W, Cn):
    """The first pixel column of every tile but the first."""
    return [k * T // Cn for k in range(1, tiles_per_row(W, Cn))]


# The 16 offsets of the corner test's circle.  No lit pixel may lie on another's: a centre with bright pixels on its circle
# is no corner.
FAST_CIRCLE = frozenset([(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1),
                         (-3, 0), (-3, 1), (-2, 2), (-1, 3)])
# centre x - b -> row - (R - 1), for x - b = -3 .. 2: rows 3 .. 9, the columns that touch the boundary on the last row of
# a row tile (R - 1) and the first row of the next (R).  The second layout is for a plane whose corner placements share
# the boundary's own column (the RGB plane with a last tile 4 pixels wide): there the first one puts pixels on their circles.
BOUNDARY_ROWS = (6, 2, 0, 1, 5, 4)
BOUNDARY_ROWS_CORNER_COLUMN = (4, 6, 5, 1, 2, 0)
BOUNDARY_FIRST_FRAME = (1, 2, 0, 3, 0, 2)


def isolated(on):
    pts = list(on)
    return all((ax - bx, ay - by) not in FAST_CIRCLE for i, (ax, ay) in enumerate(pts) for (bx, by) in pts[:i])


def edge_centres(W, Hh, Cn):
    """{(x, y): first frame}: six centres around every interior tile boundary, x - b = -3 .. 2, and the four placements
    nearest the corners.  (A centre right of W - 4 is lit like the others but can be no feature.)"""
    lo, hi_x, hi_y = FAST_BORDER, W - 1 - FAST_BORDER, Hh - 1 - FAST_BORDER
    on = {(lo, lo): 0, (hi_x, lo): 1, (lo, hi_y): 1, (hi_x, hi_y): 3}
    bs = boundaries(W, Cn)
    rows = BOUNDARY_ROWS_CORNER_COLUMN if hi_x in bs else BOUNDARY_ROWS
    for b in bs:
        for i, dx in enumerate(range(-3, 3)):
            xy = (b + dx, ROWS - 1 + rows[i])
            assert xy not in on, xy
            on[xy] = BOUNDARY_FIRST_FRAME[i]
    assert isolated(on), "a lit pixel lies on another one's corner-test circle"
    return on


def lit_clip(W, Hh, Cn, on, frames):
    """Isolated bright pixels on black (FAST corners by construction), alternating 255 / 200 from their first frame on: a lit
    pixel fires in every frame, so the feature pass looks at it in every frame."""
    clip = np.zeros((frames, Hh, W, Cn), np.uint8)
    for (x, y), k0 in on.items():
        for k in range(k0, frames):
            clip[k, y, x] = 255 if k % 2 == 0 else 200
    return clip


@functools.lru_cache(maxsize=None)
def edge_clip(W, Hh, Cn):
    c = lit_clip(W, Hh, Cn, edge_centres(W, Hh, Cn), FRAMES)
    c.setflags(write=False)
    return c


# ---- the oracle's side ----------------------------------------------------------------------------------------------
def oracle_video(W, Hh, Cn):
    """ABSOLUTE_T / Collapse, detection without rate adjustment, one row chunk (the circular event windows pair every lit
    pixel with another one, video.rs:901-903) -- the settings hip_video() gives the context."""
    ov = O.Video(W, Hh, Cn, time_mode=O.ABSOLUTE_T, multi_mode=O.COLLAPSE, ref_time=255, delta_t_max=DTM, chunk_rows=Hh)
    ov.ensure_capacity(MAX_DEPTH + 2)
    ov.set_crf_parameters(7, 7)
    ov.update_detect_features(True, False, 2, 0)
    return ov


def new_coords(ov):
    """[(x, y)] of the features the oracle's last frame found new."""
    return [(int(v) & 0xFFFF, int(v) >> 16) for v in ov.new_features()]


def oracle_display(ov, show):
    plane = ov.running_intensities()
    if show == R.SHOW_HOLD:
        ys, xs = np.nonzero(ov.feature_set())
        return R.draw_crosses(plane, list(zip(xs.tolist(), ys.tolist())))
    if show == R.SHOW_INSTANT:
        return R.draw_crosses(plane, new_coords(ov))
    return plane


class Step:
    """What the oracle holds after one frame."""

    def __init__(self, ov, events):
        self.events = events
        self.plane = ov.running_intensities()
        self.feature_set = ov.feature_set()
        self.new = new_coords(ov)
        self.display = {s: oracle_display(ov, s) for s in (R.SHOW_OFF, R.SHOW_INSTANT, R.SHOW_HOLD)}


def trace(W, Hh, Cn, clip, ov=None):
    """The clip through oracle.Video frame by frame -> [Step]; `ov` continues a video that has already seen frames."""
    ov = oracle_video(W, Hh, Cn) if ov is None else ov
    return [Step(ov, ov.integrate_matrix(f)) for f in clip]


@functools.lru_cache(maxsize=None)
def edge_trace(W, Hh, Cn):
    return trace(W, Hh, Cn, edge_clip(W, Hh, Cn))


def hip_video(A, W, Hh, Cn, show):
    """The context of the settings oracle_video() has, the plane enabled."""
    hv = A.HipVideo(W, Hh, Cn, time_mode=O.ABSOLUTE_T, multi_mode=A.MULTI_COLLAPSE, ref_time=255, delta_t_max=DTM,
                    max_depth=MAX_DEPTH, chunk_rows=Hh)
    hv.enable_running_intensities(True)
    apply_parameters(hv, show)
    return hv


def apply_parameters(hv, show):
    """The parameter calls of hip_video(), again after a reset."""
    hv.set_crf_parameters(7, 7)
    hv.update_detect_features(True, False)
    hv.set_show_features(show)


# ---- batches on the small planes: 5 + 1 + 3 frames ---------------------------------------------------------------------
BATCHES = (5, 1, 3)


@functools.lru_cache(maxsize=None)
def batch_clip(W, Hh, Cn):
    """Nine frames of bright pixels that come on one after the other, so that every batch's last frame finds a new feature
    and holds older ones (frames 4, 5 and 8 are the batches' last)."""
    on = {(3, 3): 0, (W - 4, 3): 0, (12, 9): 1, (14, 9): 2, (20, 8): 3, (20, 11): 4, (3, Hh - 4): 4, (W - 4, Hh - 4): 5,
          (9, 13): 7, (26, 6): 8, (24, 14): 8}
    c = lit_clip(W, Hh, Cn, on, sum(BATCHES))
    c.setflags(write=False)
    return c


# ---- rollback and reset: 70x37x1 ---------------------------------------------------------------------------------------
RB_PLANE = SMALL_PLANES[0]
RB_PREFIX = 3   # black frames: the context's frames_done before clip A
RB_FRAMES = 5
# A lights its pixels at batch indices 0 .. 3; B, of the same length, lights other pixels, none within a cross of A's
RB_ON_A = {(10, 8): 0, (30, 8): 0, (50, 20): 1, (16, 28): 2, (40, 30): 3}
RB_ON_B = {(20, 14): 0, (60, 10): 0, (8, 20): 1, (34, 22): 2, (58, 30): 3}


@functools.lru_cache(maxsize=None)
def rollback_clips():
    """(prefix, A, B)"""
    W, Hh, Cn = RB_PLANE
    out = (np.zeros((RB_PREFIX, Hh, W, Cn), np.uint8), lit_clip(W, Hh, Cn, RB_ON_A, RB_FRAMES), lit_clip(W, Hh, Cn, RB_ON_B, RB_FRAMES))
    for c in out:
        c.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def rollback_traces():
    """(the oracle's steps over prefix + A, over prefix + B), the prefix's steps included."""
    W, Hh, Cn = RB_PLANE
    prefix, a, b = rollback_clips()
    return trace(W, Hh, Cn, np.concatenate([prefix, a])), trace(W, Hh, Cn, np.concatenate([prefix, b]))


# ---- the per-frame ring: the `features` case of test_gpu_parity.py::test_frame_ring_submit_collect ----------------------
RING_PLANE = (131, 67, 1)
RING_FRAMES = 45
RING_IN_FLIGHT = 3


@functools.lru_cache(maxsize=None)
def ring_clip():
    import clips
    W, Hh, Cn = RING_PLANE
    c = clips.make_clip("corners", RING_FRAMES, Hh, W, Cn, seed=17)
    c.setflags(write=False)
    return c


def ring_pair(A=None):
    """(oracle.Video, HipVideo or None) of that case: rate adjustment on, radius 3, row chunks of 7."""
    W, Hh, Cn = RING_PLANE
    ov = O.Video(W, Hh, Cn, time_mode=O.ABSOLUTE_T, multi_mode=O.COLLAPSE, ref_time=255, delta_t_max=255, chunk_rows=7)
    ov.ensure_capacity(34)
    ov.set_crf_parameters(7, 7)
    ov.reset_c_thresh(2)
    ov.update_detect_features(True, True, 2, 3)
    hv = None
    if A is not None:
        hv = A.HipVideo(W, Hh, Cn, time_mode=O.ABSOLUTE_T, multi_mode=A.MULTI_COLLAPSE, ref_time=255, delta_t_max=255, chunk_rows=7,
                        max_depth=30)
        hv.set_crf_parameters(7, 7)
        hv.reset_c_thresh(2)
        hv.update_detect_features(True, True)
        hv.set_feature_parameters(2, 3)
    return ov, hv


@functools.lru_cache(maxsize=None)
def ring_trace():
    """([events per frame], the Step after the last frame, the features the frame before it found new)"""
    ov, _ = ring_pair()
    events, before = [], None
    for f in ring_clip():
        before = new_coords(ov)
        events.append(ov.integrate_matrix(f))
    return events, Step(ov, events[-1]), before


def first_difference(got, want):
    """Names the first byte of two planes [rows, width, channels] that differs."""
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    if len(bad) == 0:
        return "equal"
    y, x, c = np.unravel_index(int(bad[0]), want.shape)
    return f"{len(bad)} bytes differ, the first at byte {int(bad[0])} (x {x}, y {y}, c {c}): got {got.reshape(-1)[bad[0]]}, " \
           f"expected {want.reshape(-1)[bad[0]]}"
