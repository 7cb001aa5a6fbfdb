"""The inputs of the display-frame edge tests (tests/display_cases.py) on the CPU oracle alone: the clips put features
where the kernel's tiles meet, their crosses reach over the tile edges, Instant, Hold and Off differ, and a stamp left
behind by a refused batch has to change a display byte.  If these hold, a GPU test that compares with the same oracle
bites."""
import numpy as np
import pytest

import display_cases as D
import kernel_constants
import live_view_oracle as R


def test_constants_are_read_from_the_kernel_source():
    k = kernel_constants.display()
    assert set(k) == {"kDisplayRows", "kDisplayTileBytes"}
    assert k["kDisplayRows"] >= 1 and k["kDisplayTileBytes"] >= 16
    assert k["kDisplayTileBytes"] % 48 == 0, \
        "kDisplayTileBytes is no multiple of 48: the planes of display_cases.py assume whole RGB pixels and whole 16-byte " \
        "lines per tile"
    D.check_constants()
    # the tile counts the planes are built for
    assert [D.tiles_per_row(W, Cn) for W, _, Cn in D.PLANES] == [2, 3, 2, 3]
    assert [W * Cn - (D.tiles_per_row(W, Cn) - 1) * D.T for W, _, Cn in D.PLANES] == [5, 40, 12, 84]   # bytes of the last tile
    assert all((W * Cn) % 16 for W, _, Cn in D.PLANES)   # no row length is a whole number of lines: the rows' alignments differ
    assert (D.PLANES[0][0] * D.PLANES[0][2]) % 2 == 1      # ... and an odd one gives every row its own
    with pytest.raises(KeyError):
        kernel_constants.parse_u32_constants("constexpr uint32_t kDisplayRows = 4;", kernel_constants.DISPLAY_NAMES)


@pytest.mark.parametrize("W,H,Cn", D.PLANES, ids=D.PLANE_IDS)
def test_members_and_crosses_on_both_sides_of_every_tile_boundary(W, H, Cn):
    steps = D.edge_trace(W, H, Cn)
    last = steps[-1]
    # the crosses are looked at in a frame whose lit pixels are 200, not 255: there a cross changes every byte it covers
    assert D.FRAMES % 2 == 1 and set(np.unique(D.edge_clip(W, H, Cn)[-2])) == {0, 200}
    assert np.array_equal(steps[-2].feature_set, last.feature_set)
    fs, hold, plane = last.feature_set, steps[-2].display[R.SHOW_HOLD], steps[-2].plane
    bs = D.boundaries(W, Cn)
    assert len(bs) == D.tiles_per_row(W, Cn) - 1 >= 1
    for b in bs:
        # the corner test admits centres up to column W - 4: in the RGB plane whose last tile is 4 pixels wide that is the
        # boundary's own column, and no feature can exist right of it
        cols = [x for x in (b - 2, b - 1, b, b + 1) if x <= W - 1 - D.FAST_BORDER]
        assert cols[:3] == [b - 2, b - 1, b], (b, cols)
        assert len(cols) == 4 or (W, Cn) == (D.T // 3 + 4, 3), (b, cols)
        for x in cols:
            ys = np.flatnonzero(fs[:, x])
            assert len(ys), f"no member in column {x} at boundary {b}"
            for y in ys:   # its cross changes bytes left and right of the boundary
                row_changed = np.flatnonzero((hold[y] != plane[y]).any(axis=1))
                arm = row_changed[(row_changed >= x - D.CROSS_REACH) & (row_changed <= x + D.CROSS_REACH)]
                assert (arm < b).any() and (arm >= b).any(), (b, x, int(y), arm)
    assert fs[D.ROWS - 1].any() and fs[D.ROWS].any()   # members on the last row of a row tile and the first of the next
    # the four placements nearest the corners
    assert fs[3, 3] and fs[3, W - 4] and fs[H - 4, 3] and fs[H - 4, W - 4]
    # every lit pixel the corner test admits is a feature, and nothing else is
    want = np.zeros_like(fs)
    for (x, y) in D.edge_centres(W, H, Cn):
        if x <= W - 1 - D.FAST_BORDER:
            want[y, x] = 1
    assert np.array_equal(fs, want)


@pytest.mark.parametrize("W,H,Cn", D.PLANES + D.SMALL_PLANES)
def test_instant_hold_and_off_differ(W, H, Cn):
    steps = D.edge_trace(W, H, Cn) if (W, H, Cn) in D.PLANES else D.trace(W, H, Cn, D.batch_clip(W, H, Cn))
    assert any(not np.array_equal(s.display[R.SHOW_INSTANT], s.display[R.SHOW_HOLD]) and
               not np.array_equal(s.display[R.SHOW_INSTANT], s.plane) for s in steps)
    assert all(np.array_equal(s.display[R.SHOW_OFF], s.plane) for s in steps)
    assert not np.array_equal(steps[-1].display[R.SHOW_HOLD], steps[-1].plane)
    assert len({len(s.new) for s in steps}) > 2   # the features come in different frames


@pytest.mark.parametrize("W,H,Cn", D.SMALL_PLANES)
def test_every_batch_ends_on_a_frame_with_new_and_held_features(W, H, Cn):
    steps = D.trace(W, H, Cn, D.batch_clip(W, H, Cn))
    assert len(steps) == sum(D.BATCHES)
    end = 0
    for n in D.BATCHES:
        end += n
        s = steps[end - 1]
        assert s.new and s.feature_set.sum() > len(s.new), end - 1
        assert not np.array_equal(s.display[R.SHOW_INSTANT], s.display[R.SHOW_HOLD])
        assert not np.array_equal(s.display[R.SHOW_INSTANT], s.plane)
    # a stamp one frame off shows: the frame before a batch's last frame found other features new, or none
    assert steps[3].new != steps[4].new and steps[7].new != steps[8].new


def _near(p, q):
    return abs(p[0] - q[0]) <= D.CROSS_REACH and abs(p[1] - q[1]) <= D.CROSS_REACH


def test_a_stale_stamp_changes_a_display_byte():
    """Some pixel P is new at A's frame k, while in the run that never saw A P is not new at B's frame k and lies under no
    cross of a pixel that is: a stamp the refused batch left at P is drawn on bytes that the oracle leaves alone."""
    prefix, a, b = D.rollback_clips()
    ta, tb = D.rollback_traces()
    F = len(prefix)
    assert len(a) == len(b) == D.RB_FRAMES and len(ta) == len(tb) == F + D.RB_FRAMES
    assert all(not s.new and not s.feature_set.any() for s in ta[:F])
    found = []
    for k in range(D.RB_FRAMES):
        for p in ta[F + k].new:
            if p not in tb[F + k].new and not any(_near(p, q) for q in tb[F + k].new):
                stale = R.draw_crosses(tb[F + k].display[R.SHOW_INSTANT], [p])
                assert not np.array_equal(stale, tb[F + k].display[R.SHOW_INSTANT])
                found.append((k, p))
    assert len({k for k, _ in found}) >= 3, found   # at several batch indices, the first included
    assert found[0][0] <= 1
    # B's own features are all new somewhere, so Instant shows something in the clean run as well
    assert sum(len(s.new) for s in tb[F:]) == len(D.RB_ON_B) and sum(len(s.new) for s in ta[F:]) == len(D.RB_ON_A)
    # the batch that is refused holds events in its last frame, so a buffer one event short cuts that frame
    assert len(ta[F + D.RB_FRAMES - 1].events) > 0


def test_the_ring_case_ends_on_new_features():
    _, last, before = D.ring_trace()
    assert last.new and last.feature_set.sum() > len(last.new)
    assert set(before) != set(last.new)   # (a stamp one frame off shows)
    assert not np.array_equal(last.display[R.SHOW_INSTANT], last.plane)
    assert not np.array_equal(last.display[R.SHOW_INSTANT], last.display[R.SHOW_HOLD])


def test_stamps_that_survive_a_reset_change_a_display_byte():
    """Clip A, then clip B from the start: a pixel that A made new at frame k is not new in B's frame k, nor under a cross."""
    W, H, Cn = D.RB_PLANE
    _, a, b = D.rollback_clips()
    ta, tb = D.trace(W, H, Cn, a), D.trace(W, H, Cn, b)
    found = [(k, p) for k in range(D.RB_FRAMES) for p in ta[k].new
             if p not in tb[k].new and not any(_near(p, q) for q in tb[k].new)]
    assert len({k for k, _ in found}) >= 3, found
    assert sum(len(s.new) for s in tb) == len(D.RB_ON_B)
