"""Region balloons (csrc/balloon.hip, include/tsii_hip.h "K25: region balloons") through the C ABI on the emulator (CPU suite) and, with
-m gpu, on the chip: per table row the flood fill from the row's own text over the ring's colour, its area, box and open flag, the anchor
and the largest upright rectangle around it.

Every comparison is integer EQUALITY with a restatement that shares no code with the kernels (which work on bit planes of the window):
per region a max-pool dilation for the ring, ``min`` / ``max`` / ``sum`` in Python integers, a queue-based flood fill over boolean arrays
and brute-force loops for the anchor and the rectangle.  The rectangle is checked twice: by the header's definition (``balloon_ref``) and,
on the small pages, by an exhaustive search over ALL upright rectangles inside the balloon that hold the anchor (``largest_rectangle``):
their agreement is the independent evidence for the header's candidate argument.  The ring's colour and count are also compared with
``tsii_flat_regions`` on the same inputs.  Labels and tables come from ``tsii_text_regions`` on the device; every output carries a canary
tail, the rows behind ``R`` are canaries, the workspace is handed over full of canary bytes.
"""
import collections
import functools

import numpy as np
import pytest
import torch

from tests.backends import BACKENDS, both_backends
from tests.test_flat_kernels import Flat
from tests.test_pipeline_kernels import Buf, up
from tests.test_text_eraser import dilate_np
from tests.test_text_regions import CANARY32, HALO, TILE, Planes, expected, pattern
from text_segmentation_image_inpainting_amd import _lib
from text_segmentation_image_inpainting_amd.pipeline import tile_grid

CANARY64 = int(np.frombuffer(bytes([0xA5] * 8), np.int64)[0])
PAPER, WALL, INK = (200, 210, 220), (30, 60, 90), (0, 0, 0)


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def flood_runs(passable, seeds):
    """the same set by whole runs: every run of ``passable`` along a row that holds a seen pixel becomes seen, then every run along a
    column, until nothing is added.  numpy only; what the one large window uses instead of a Python queue of 600000 pixels"""
    seen = seeds & passable
    while True:
        before = int(seen.sum())
        for turn in (False, True):
            P, S = (passable.T, seen.T) if turn else (passable, seen)
            start = P & ~np.pad(P, ((0, 0), (1, 0)))[:, :-1]
            ids = np.cumsum(start.reshape(-1)).reshape(P.shape)          # the number of the run a passable pixel lies in
            hit = np.zeros(int(ids.max()) + 1, bool)
            hit[ids[S]] = True
            S = P & hit[ids]
            seen = S.T if turn else S
        if int(seen.sum()) == before:
            return seen


def flood(passable, seeds):
    """the 4-connected components of ``passable`` that hold a seed: a queue; the small planes check ``flood_runs`` against it"""
    h, w = passable.shape
    if passable.size > 200000:
        return flood_runs(passable, seeds)
    seen = seeds & passable
    queue = collections.deque(zip(*np.nonzero(seen)))
    while queue:
        y, x = queue.popleft()
        for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= yy < h and 0 <= xx < w and passable[yy, xx] and not seen[yy, xx]:
                seen[yy, xx] = True
                queue.append((yy, xx))
    assert np.array_equal(seen, flood_runs(passable, seeds)), "the two restatements of the fill disagree"
    return seen


def run_ends(row, x):
    a = b = x
    while a > 0 and row[a - 1]:
        a -= 1
    while b + 1 < len(row) and row[b + 1]:
        b += 1
    return a, b


def defined_rectangle(B, ay, ax):
    """the header's definition, window coordinates: (ya, max L, yb + 1, min Rr + 1)"""
    top = ay
    while top > 0 and B[top - 1, ax]:
        top -= 1
    bot = ay
    while bot + 1 < B.shape[0] and B[bot + 1, ax]:
        bot += 1
    ends = {y: run_ends(B[y], ax) for y in range(top, bot + 1)}
    best = None
    for ya in range(top, ay + 1):
        L0, R0 = max(ends[y][0] for y in range(ya, ay + 1)), min(ends[y][1] for y in range(ya, ay + 1))
        for yb in range(ay, bot + 1):
            L, Rr = L0, R0 = max(L0, ends[yb][0]), min(R0, ends[yb][1])
            key = (-(yb - ya + 1) * (Rr - L + 1), ya, yb)
            if best is None or key < best[0]:
                best = (key, (ya, L, yb + 1, Rr + 1))
    return best[1]


def largest_rectangle(B, ay, ax):
    """the area of the largest upright rectangle inside B that holds (ay, ax): every rectangle is tried (integral image)"""
    h, w = B.shape
    S = np.zeros((h + 1, w + 1), np.int64)
    S[1:, 1:] = np.cumsum(np.cumsum(B.astype(np.int64), axis=0), axis=1)
    xa, xb = np.arange(0, ax + 1)[:, None], np.arange(ax + 1, w + 1)[None, :]
    best = 0
    for ya in range(0, ay + 1):
        for yb in range(ay + 1, h + 1):
            inside = S[yb, xb] - S[ya, xb] - S[yb, xa] + S[ya, xa]
            full = (yb - ya) * (xb - xa)
            best = max(best, int(np.where(inside == full, full, 0).max()))
    return best


def balloon_ref(page, text, labels, table, R, ring, tol, reach, exhaustive=False):
    """-> (balloon rows [R, 16], rect rows [R, 8] int64, plane [h, w], the balloons as boolean page planes)"""
    h, w = text.shape
    text01 = text != 0
    rows, rect, plane, balloons = np.zeros((R, 16), np.int64), np.zeros((R, 8), np.int64), np.zeros((h, w), np.uint8), []
    for r in range(R):
        balloons.append(None)
        lab = int(table[r][0])
        y0, x0, y1, x1 = (min(max(int(v), 0), lim) for v, lim in zip(table[r][2:6], (h, w, h, w)))
        wy0, wx0, wy1, wx1 = max(y0 - reach, 0), max(x0 - reach, 0), min(y1 + reach, h), min(x1 + reach, w)
        if wy1 - wy0 > 1024 or wx1 - wx0 > 1024:
            rows[r, 0] = 8
            continue
        own = np.zeros((h, w), bool)
        if y0 < y1 and x0 < x1:
            own[y0:y1, x0:x1] = (labels[y0:y1, x0:x1] == lab) & text01[y0:y1, x0:x1]
        if not own.any():
            rows[r, 0] = 16
            continue
        win = (slice(wy0, wy1), slice(wx0, wx1))
        ringm = (dilate_np(own[win], 2 * ring + 1) != 0) & ~text01[win]
        n = int(ringm.sum())
        status, colour = 0, [0, 0, 0]
        if n == 0:
            status = 1
        else:
            px = page[win][ringm].astype(np.int64)
            colour = [(2 * int(v) + n) // (2 * n) for v in px.sum(axis=0)]
            if ((px.max(axis=0) - px.min(axis=0)) > tol).any():
                status |= 2
        ay, ax = min(zip(*np.nonzero(own)), key=lambda p: (abs(2 * p[0] - (y0 + y1 - 1)) + abs(2 * p[1] - (x0 + x1 - 1)), p[0], p[1]))
        rows[r, :5], rows[r, 10:12] = [status, n] + colour, (ay, ax)
        if status:
            continue
        near = (np.abs(page[win].astype(np.int64) - np.array(colour)) <= tol).all(axis=-1)
        B = flood(own[win] | (~text01[win] & near), own[win])
        ys, xs = np.nonzero(B)
        open_ = (wy0 > 0 and B[0].any()) or (wy1 < h and B[-1].any()) or (wx0 > 0 and B[:, 0].any()) or (wx1 < w and B[:, -1].any())
        ra = defined_rectangle(B, ay - wy0, ax - wx0)
        if exhaustive:
            assert (ra[2] - ra[0]) * (ra[3] - ra[1]) == largest_rectangle(B, ay - wy0, ax - wx0)
        assert B[ra[0]:ra[2], ra[1]:ra[3]].all()
        ry0, rx0, ry1, rx1 = ra[0] + wy0, ra[1] + wx0, ra[2] + wy0, ra[3] + wx0
        rows[r, 0] = 4 if open_ else 0
        rows[r, 5:10] = (len(ys), ys.min() + wy0, xs.min() + wx0, ys.max() + 1 + wy0, xs.max() + 1 + wx0)
        rows[r, 12:16] = (ry0, rx0, ry1, rx1)
        rect[r] = (-1, 0, 1, rx0, rx1 - 1, -(ry1 - 1), -ry0, 1)
        full = np.zeros((h, w), bool)
        full[win] = B
        balloons[r] = full
        plane[full] = 255
    return rows, rect, plane, balloons


# ---- the kernels -----------------------------------------------------------------------------------------------------------------
class Balloons:
    """the extra buffers of one tsii_region_balloons call behind a ``Planes`` of tests/test_text_regions.py"""

    def __init__(self, dev, planes, page, reach):
        self.p, n = planes, planes.h * planes.w
        self.page = up(dev, page)
        self.rows, self.rect = Buf(dev, 16 * planes.max_regions, torch.int32), Buf(dev, 8 * planes.max_regions, torch.int64)
        self.plane = Buf(dev, n, torch.uint8)
        nbytes = _lib.lib().tsii_region_balloons_ws_bytes(planes.h, planes.w, planes.max_regions, reach)
        assert nbytes > 0 and nbytes % 4 == 0
        self.ws = Buf(dev, nbytes // 4, torch.int32)

    def run(self, ring, tol, reach, plane=True, **bad):
        p = self.p
        a = dict(page=_lib.ptr(self.page), text=p.text.ptr, labels=p.labels.ptr, h=p.h, w=p.w, table=p.table.ptr, n=p.n.ptr,
                 max_regions=p.max_regions, ring=ring, tol=tol, reach=reach, rows=self.rows.ptr, rect=self.rect.ptr,
                 plane=self.plane.ptr if plane else None, ws=self.ws.ptr)
        a.update(bad)
        _lib.call("tsii_region_balloons", a["page"], a["text"], a["labels"], a["h"], a["w"], a["table"], a["n"], a["max_regions"], a["ring"],
                  a["tol"], a["reach"], a["rows"], a["rect"], a["plane"], a["ws"], _lib.stream())

    def get(self):
        ws = self.ws.get()
        p = self.p
        return (self.rows.get().reshape(-1, 16), self.rect.get().reshape(-1, 8), self.plane.get().reshape(p.h, p.w), ws[-p.max_regions:])


def untouched(a):
    return bool((np.asarray(a).reshape(-1).view(np.uint8) == 0xA5).all())


def run_page(backend, page, text, ring, tol, reach, max_regions=None, connectivity=8, plane=True, exhaustive=False, flat=True):
    """one call behind tsii_text_regions -> (reference rows, the balloons, the device's sweeps): everything already compared"""
    h, w = text.shape
    g = tile_grid(h, w, TILE, HALO)
    exp = expected(text, connectivity, 0, g)
    max_regions = exp["n"][1] + 2 if max_regions is None else max_regions
    R = min(exp["n"][1], max_regions)
    rows, rect, ref_plane, balloons = balloon_ref(page, exp["text"], exp["labels"], exp["table"], R, ring, tol, reach, exhaustive)
    with BACKENDS[backend]() as dev:
        planes = Planes(dev, text, max_regions, g)
        planes.run(connectivity, 0)
        before = planes.get()
        b = Balloons(dev, planes, page, reach)
        b.run(ring, tol, reach, plane=plane)
        got_rows, got_rect, got_plane, sweeps = b.get()
        after = planes.get()
        page_after = b.page.cpu().numpy()
        flat_rows = None
        if flat:
            fl = Flat(dev, planes, page)
            fl.run(ring, tol)
            flat_rows = fl.get()[3]
    for key in ("labels", "table", "n", "text"):
        assert np.array_equal(np.asarray(before[key]), np.asarray(after[key])), f"{key} is read only"
    assert np.array_equal(page_after, page), "the page is read only"
    assert np.array_equal(got_rows[:R], rows), (got_rows[:R], rows)
    assert np.array_equal(got_rect[:R], rect), (got_rect[:R], rect)
    assert untouched(got_rows[R:]) and untouched(got_rect[R:]), "rows behind R must not be touched"
    assert np.array_equal(got_plane, ref_plane) if plane else untouched(got_plane)
    if flat:                                            # K13 on the same inputs: the colour and the count of every row that has a ring
        for r in range(R):
            if not rows[r, 0] & (8 | 16):
                assert list(flat_rows[r][1:5]) == list(rows[r, 2:5]) + [rows[r, 1]], (r, flat_rows[r], rows[r])
    return rows, balloons, sweeps[:R]


def noise_page(h, w, seed=5):
    return np.random.default_rng(seed + h).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def scene(passable, text, h=None, w=None, at=(0, 0), outside=None):
    """a page of WALL with PAPER where ``passable`` and INK where ``text``, the masks laid at ``at`` on a page of h x w"""
    mh, mw = passable.shape
    h, w = h or mh, w or mw
    page = np.empty((h, w, 3), np.uint8)
    page[:] = WALL if outside is None else outside
    plane = np.zeros((h, w), np.uint8)
    sub = page[at[0]:at[0] + mh, at[1]:at[1] + mw]
    sub[:] = WALL
    sub[passable] = PAPER
    sub[text] = INK
    plane[at[0]:at[0] + mh, at[1]:at[1] + mw][text] = 7
    return page, plane


def ellipse_page(h, w):
    """an ellipse of one colour with a block in it on noise, a second block out in the noise"""
    yy, xx = np.mgrid[0:h, 0:w]
    page = noise_page(h, w)
    inside = ((yy - h * 0.5) / (h * 0.36)) ** 2 + ((xx - w * 0.45) / (w * 0.4)) ** 2 <= 1.0
    page[inside] = PAPER
    text = np.zeros((h, w), np.uint8)
    text[h // 2 - 3:h // 2 + 2, int(w * 0.45) - 4:int(w * 0.45) + 5] = 9
    text[h // 2 - 2, int(w * 0.45)] = 0                                 # a hole in the lettering: not text, of the paper's colour
    text[1:4, w - 6:w - 2] = 9
    page[text != 0] = INK
    return page, text


# ---- tests -----------------------------------------------------------------------------------------------------------------------
@both_backends
@pytest.mark.parametrize("hw,reach,closed", [((40, 50), 64, True), ((40, 50), 6, False), ((150, 217), 40, False), ((150, 217), 256, True)])
def test_ellipse_on_noise(backend, hw, reach, closed):
    page, text = ellipse_page(*hw)
    rows, balloons, _ = run_page(backend, page, text, 3, 8, reach, exhaustive=hw == (40, 50))
    assert rows[0, 0] == 2, "the block in the noise has no colour around it"
    assert rows[1, 0] == (0 if closed else 4) and rows[1, 5] > 0
    if closed:
        assert rows[1, 5] == int((page == PAPER).all(axis=-1).sum()) + int((text[hw[0] // 2 - 5:hw[0] // 2 + 5] != 0).sum())


@both_backends
@pytest.mark.parametrize("shift", [0, 1, 2, 31])
def test_word_boundaries(backend, shift):
    """a balloon from x = 20 to 75 in a window that starts at x = 6 + shift: its runs cross the words' ends both ways"""
    passable = np.zeros((30, 130), bool)
    passable[4:26, 20 + shift:76 + shift] = True
    passable[10:12, 30 + shift:70 + shift] = False                       # a bar: two arms joined through other words
    text = np.zeros_like(passable)
    text[15:18, 46 + shift:50 + shift] = True
    rows, _, _ = run_page(backend, *scene(passable, text), 2, 10, 40, exhaustive=True)
    assert rows[0, 0] == 0 and rows[0, 5] == 22 * 56 - 2 * 40


@both_backends
def test_four_corners(backend):
    """windows clipped by the page in every corner: the page's edge closes a balloon"""
    h, w = 60, 90
    passable = np.zeros((h, w), bool)
    text = np.zeros((h, w), bool)
    for ys, xs in ((slice(0, 14), slice(0, 20)), (slice(0, 14), slice(w - 20, w)), (slice(h - 14, h), slice(0, 20)), (slice(h - 14, h), slice(w - 20, w))):
        passable[ys, xs] = True
        text[ys, xs][5:8, 7:12] = True
    rows, _, _ = run_page(backend, *scene(passable, text), 3, 4, 30, exhaustive=True)
    assert (rows[:, 0] == 0).all() and (rows[:, 5] == 14 * 20).all()


def spiral(n):
    """a chamber of 5 x 5 in the middle of n x n and a one-pixel corridor that winds outwards from it, two pixels between its turns"""
    m = np.zeros((n, n), bool)
    c = n // 2
    m[c - 2:c + 3, c - 2:c + 3] = True
    y, x, dy, dx, step = c, c + 2, 0, 1, 6
    while True:
        for _ in range(step):
            y, x = y + dy, x + dx
            if not (1 <= y < n - 1 and 1 <= x < n - 1):
                return m
            m[y, x] = True
        dy, dx = dx, -dy
        step += 2


@both_backends
def test_spiral_corridor(backend):
    passable = spiral(45)
    text = np.zeros_like(passable)
    text[22, 22] = True
    rows, _, sweeps = run_page(backend, *scene(passable, text, 70, 80, at=(12, 20)), 1, 0, 40)
    assert rows[0, 0] == 0 and rows[0, 5] == int(passable.sum()) and sweeps[0] > 3


@both_backends
def test_u_and_arms(backend):
    """the text at the bottom of a U: both arms are reached upwards; a third arm hangs from a bridge in the next word"""
    passable = np.zeros((50, 90), bool)
    passable[40:46, 4:80] = True                                        # the bottom
    passable[3:40, 4:8] = passable[3:40, 28:31] = True                  # two arms up
    passable[3:6, 28:70] = True                                         # a bridge at the top, to the right, across two words
    passable[6:30, 66:70] = True                                        # and an arm down from it
    text = np.zeros_like(passable)
    text[42:44, 10:16] = True
    rows, _, _ = run_page(backend, *scene(passable, text), 1, 0, 80)
    assert rows[0, 5] == int(passable.sum())


def boxed(gap):
    passable = np.ones((40, 60), bool)
    passable[10, 15:45] = passable[30, 15:45] = passable[10:31, 15] = passable[10:31, 44] = False       # a one-pixel outline
    if gap == "diagonal":
        passable[10, 43:45] = True                                      # the corner cut off: (10, 43), (10, 44) open, (11, 44) a wall:
        passable[11, 43] = False                                        # inside (11, 42) meets (10, 43) only across a diagonal
    elif gap == "true":
        passable[20, 44] = True
    text = np.zeros_like(passable)
    text[19:22, 27:33] = True
    return passable, text


@both_backends
@pytest.mark.parametrize("gap", ["none", "diagonal", "true"])
def test_outline_gaps(backend, gap):
    passable, text = boxed(gap)
    rows, _, _ = run_page(backend, *scene(passable, text, 60, 80, at=(10, 10), outside=PAPER), 2, 0, 24)
    inside = 19 * 28 - (1 if gap == "diagonal" else 0)
    if gap == "true":
        assert rows[0, 0] == 4 and rows[0, 5] > inside, "a true gap leaks: the balloon is open"
    else:
        assert rows[0, 0] == 0 and rows[0, 5] == inside, "a diagonal gap does not leak at 4-connectivity"


@both_backends
@pytest.mark.parametrize("channel", [0, 1, 2])
@pytest.mark.parametrize("over", [0, 1])
@pytest.mark.parametrize("where", ["ring", "passable"])
def test_tolerance_bounds(backend, where, over, channel):
    tol = 9
    passable = np.zeros((30, 40), bool)
    passable[5:25, 5:35] = True
    text = np.zeros_like(passable)
    text[14:16, 18:22] = True
    page, plane = scene(passable, text)
    y, x = (13, 20) if where == "ring" else (8, 30)
    page[y, x, channel] += tol + over
    rows, _, _ = run_page(backend, page, plane, 1, tol, 30, exhaustive=True)
    if where == "ring":
        assert rows[0, 0] == (2 if over else 0)
    else:
        assert rows[0, 0] == 0 and rows[0, 5] == 20 * 30 - over


@both_backends
def test_two_blocks_in_one_balloon(backend):
    passable = np.zeros((40, 70), bool)
    passable[4:36, 4:66] = True
    text = np.zeros_like(passable)
    text[10:14, 12:30] = True
    text[24:30, 30:56] = True
    page, plane = scene(passable, text)
    rows, balloons, _ = run_page(backend, page, plane, 2, 0, 64, exhaustive=True)
    assert (rows[:, 0] == 0).all()
    paper = int(passable.sum()) - int(text.sum())
    assert rows[0, 5] == paper + 4 * 18 and rows[1, 5] == paper + 6 * 26, "the shared paper counts in both, the neighbour's text in neither"
    for r, other in ((0, text[24:30, 30:56]), (1, text[10:14, 12:30])):
        ry0, rx0, ry1, rx1 = rows[r, 12:16]
        own = np.zeros_like(text)
        own[ry0:ry1, rx0:rx1] = True
        assert not (own & (text & ~balloons[r])).any(), "the inner rectangle keeps off the neighbour's lettering"


@both_backends
@pytest.mark.parametrize("ring,reach", [(3, 3), (2, 10), (8, 8)])
def test_bare_paper_is_open(backend, ring, reach):
    page = np.empty((60, 70, 3), np.uint8)
    page[:] = PAPER
    text = np.zeros((60, 70), np.uint8)
    text[25:30, 30:42] = 1
    page[text != 0] = INK
    rows, _, _ = run_page(backend, page, text, ring, 0, reach, exhaustive=True)
    assert rows[0, 0] == 4 and rows[0, 5] == (5 + 2 * reach) * (12 + 2 * reach), "the window, the own text included"


@both_backends
def test_reach_512_on_a_small_page(backend):
    page, text = ellipse_page(40, 50)
    run_page(backend, page, text, 3, 8, 512)


@both_backends
def test_no_ring_and_mixed_ring(backend):
    rows, _, _ = run_page(backend, noise_page(12, 9), pattern("full", 12, 9), 3, 255, 8)
    assert rows[0, 0] == 1 and not rows[0, 1:10].any()
    rows, _, _ = run_page(backend, noise_page(40, 50), pattern("noise0.3", 40, 50), 2, 30, 16)
    assert (rows[:, 0] == 2).any()


@both_backends
def test_window_too_large(backend):
    page = np.full((4, 1200, 3), 200, np.uint8)
    text = np.zeros((4, 1200), np.uint8)
    text[1, 50:1150] = 1                                                 # its box is wider than 1024
    text[3, 5:8] = 1                                                     # a small one beside it
    rows, _, _ = run_page(backend, page, text, 1, 0, 16)
    assert rows[0, 0] == 8 and not rows[0, 1:].any() and rows[1, 0] in (0, 4)


@both_backends
def test_plus_shaped_balloon_ties(backend):
    """a plus of two bars of equal area: the candidates tie, the smaller ya wins; an anchor tie goes to the smallest y, then x"""
    passable = np.zeros((41, 41), bool)
    passable[5:36, 16:25] = passable[16:25, 5:36] = True
    text = np.zeros_like(passable)
    text[19:21, 19:21] = True                                            # four pixels at the same distance from the centre
    rows, _, _ = run_page(backend, *scene(passable, text), 1, 0, 41, exhaustive=True)
    assert tuple(rows[0, 10:12]) == (19, 19)
    assert tuple(rows[0, 12:16]) == (5, 16, 36, 25), "the upright bar starts higher"


@both_backends
def test_truncated_table_and_null_plane(backend):
    page, text = ellipse_page(40, 50)
    text[30:33, 20:26] = 9                                               # a second block in the ellipse, behind max_regions
    page[30:33, 20:26] = INK
    rows, _, _ = run_page(backend, page, text, 2, 8, 64, max_regions=2, plane=False)
    assert rows[1, 0] == 0
    assert rows[1, 5] == int((page == PAPER).all(axis=-1).sum()) + int((text[15:25] != 0).sum()), "the third block is still an obstacle"


@both_backends
@pytest.mark.parametrize("name,hw,tol", [("noise0.3", (40, 50), 255), ("noise0.45", (40, 50), 100), ("noise0.3", (70, 90), 255)])
def test_noise_planes(backend, name, hw, tol):
    page = noise_page(*hw) if tol < 255 else (noise_page(*hw) // 2 + 60)
    rows, _, _ = run_page(backend, page, pattern(name, *hw), 1, tol, 12, connectivity=4)
    assert len(rows) > 20


@both_backends
def test_window_above_the_lds_planes(backend):
    """a window of 25 words x 800 rows: the passable plane lives in the workspace"""
    h, w = 800, 790
    page = np.empty((h, w, 3), np.uint8)
    page[:] = PAPER
    page[:, 600:602] = WALL                                              # a wall with a door: the fill has to turn
    page[700:702, 600:602] = PAPER
    text = np.zeros((h, w), np.uint8)
    text[398:402, 300:310] = 1
    page[text != 0] = INK
    rows, _, sweeps = run_page(backend, page, text, 2, 0, 512, flat=False)
    assert rows[0, 0] == 0 and rows[0, 5] == h * w - 2 * (h - 2) and sweeps[0] >= 2


@both_backends
def test_rectangle_through_crops_and_paste(backend):
    """rect fed to tsii_region_crops at the rectangle's own size gives the page's bytes of the rectangle, and through tsii_region_paste an
    opaque slot changes exactly the rectangle's pixels, to the slot's bytes: an off-by-one in the signed dot products of rect would show"""
    from tests.test_region_crops import Crops
    from tests.test_region_paste import Paste
    page, text = ellipse_page(40, 50)
    page[(page == PAPER).all(axis=-1)] += np.random.default_rng(1).integers(0, 5, size=(int((page == PAPER).all(axis=-1).sum()), 3), dtype=np.uint8)
    exp = expected(text, 8, 0, None)
    rows, rect, _, _ = balloon_ref(page, exp["text"], exp["labels"], exp["table"], 2, 3, 8, 64)
    ry0, rx0, ry1, rx1 = (int(v) for v in rows[1, 12:16])
    assert (ry0, rx0, ry1, rx1) == (-int(rect[1, 6]), int(rect[1, 3]), -int(rect[1, 5]) + 1, int(rect[1, 4]) + 1) and ry1 - ry0 > 3 and rx1 - rx0 > 3
    slot = np.full((1, ry1 - ry0, rx1 - rx0, 4), 255, np.uint8)
    slot[0, :, :, :3] = page[ry0:ry1, rx0:rx1] + np.uint8(97)           # every byte differs from the page's
    with BACKENDS[backend]() as dev:
        planes = Planes(dev, text, 4, None)
        planes.run(8, 0)
        b = Balloons(dev, planes, page, 64)
        b.run(3, 8, 64)
        got = b.get()[1]
        assert np.array_equal(got[:2], rect)
        c = Crops(dev, page, got[1:2].copy(), 1, 1, 1, ry1 - ry0, rx1 - rx0)
        c.run()
        info, crops = c.get()
        p = Paste(dev, page, info[:1].copy(), 1, 1, slot)
        p.run()
        plan, pasted = p.get()
    assert tuple(info[0][:2]) == (ry1 - ry0, rx1 - rx0)
    assert np.array_equal(crops[0], page[ry0:ry1, rx0:rx1])
    inside = np.zeros(page.shape[:2], bool)
    inside[ry0:ry1, rx0:rx1] = True
    assert plan[0, 0] == 1 and np.array_equal((pasted != page).any(axis=-1), inside), "exactly the rectangle's pixels change"
    assert np.array_equal(pasted[ry0:ry1, rx0:rx1], slot[0, :, :, :3]) and np.array_equal(pasted[~inside], page[~inside])


class BlockPlanes:
    """what ``Balloons`` reads of a ``Planes``, of the buffers tsii_text_blocks left (tests/test_text_blocks_kernels.py)"""

    def __init__(self, blocks):
        self.h, self.w, self.max_regions = blocks.h, blocks.w, blocks.max_regions
        self.text, self.labels, self.table, self.n = blocks.text, blocks.blocks, blocks.table, blocks.n


@both_backends
def test_on_the_blocks_of_text_blocks(backend):
    """the table and the labels of tsii_text_blocks: a block of two glyphs is one row, its own glyphs are no obstacle to it"""
    from tests.test_text_blocks_kernels import Planes as Blocks, check as check_blocks, expected as expected_blocks, k10_labels
    page, text = ellipse_page(40, 50)
    h, w = text.shape
    gap_x = int(w * 0.45)
    text[h // 2 - 3:h // 2 + 2, gap_x] = 0                               # the block falls into two glyphs one pixel apart
    page[h // 2 - 3:h // 2 + 2, gap_x] = PAPER
    labels = k10_labels(text)
    exp = expected_blocks(text, labels, 2, 0, None)
    assert exp["n"] == (2, 2) and list(exp["members"]) == [1, 2]
    max_regions = 5
    rows, rect, ref_plane, _ = balloon_ref(page, exp["text"], exp["labels"], exp["table"], 2, 3, 8, 64, exhaustive=True)
    with BACKENDS[backend]() as dev:
        blocks = Blocks(dev, text, labels, 2, max_regions, None)
        blocks.run()
        check_blocks(blocks.get(), exp, max_regions, labels)
        b = Balloons(dev, BlockPlanes(blocks), page, 64)
        b.run(3, 8, 64)
        got_rows, got_rect, got_plane, _ = b.get()
        check_blocks(blocks.get(), exp, max_regions, labels)                # all of it is read only
    assert np.array_equal(got_rows[:2], rows) and np.array_equal(got_rect[:2], rect) and np.array_equal(got_plane, ref_plane)
    assert untouched(got_rows[2:]) and untouched(got_rect[2:])
    assert rows[1, 0] == 0 and rows[1, 5] == int((page == PAPER).all(axis=-1).sum()) + int((text[h // 2 - 5:h // 2 + 5] != 0).sum())


@both_backends
def test_refusals(backend):
    page, text = ellipse_page(40, 50)
    with BACKENDS[backend]() as dev:
        planes = Planes(dev, text, 4, None)
        planes.run(8, 0)
        b = Balloons(dev, planes, page, 64)
        bad = [dict(h=0), dict(w=0), dict(h=32768), dict(max_regions=0), dict(ring=0), dict(ring=9), dict(tol=-1), dict(tol=256),
               dict(reach=2, ring=3), dict(reach=513), dict(page=None), dict(text=None), dict(labels=None), dict(table=None), dict(n=None),
               dict(rows=None), dict(rect=None), dict(ws=None), dict(rect=_lib.ctypes.c_void_p(b.rect.ptr.value + 4)),
               dict(ws=_lib.ctypes.c_void_p(b.ws.ptr.value + 2)), dict(rows=_lib.ctypes.c_void_p(b.rows.ptr.value + 2)), dict(w=32768)]
        for kw in bad:
            with pytest.raises(RuntimeError, match="region_balloons"):
                b.run(**{**dict(ring=3, tol=8, reach=64), **kw})
        rows, rect, plane, _ = b.get()
        assert untouched(rows) and untouched(rect) and untouched(plane), "a refused call writes nothing"
        assert untouched(b.ws.get())
        lib = _lib.lib()
        assert lib.tsii_region_balloons_ws_bytes(0, 5, 4, 64) == 0 and lib.tsii_region_balloons_ws_bytes(5, 5, 0, 64) == 0
        assert lib.tsii_region_balloons_ws_bytes(5, 5, 4, 0) == 0 and lib.tsii_region_balloons_ws_bytes(5, 5, 4, 513) == 0
        assert lib.tsii_region_balloons_ws_bytes(32768, 5, 4, 64) == 0 and lib.tsii_region_balloons_ws_bytes(5, 32768, 4, 64) == 0
        assert lib.tsii_region_balloons_ws_bytes(32767, 32767, 4, 64) > 0, "the largest page the sides allow: h * w <= 2^31 - 2 follows from them"


def test_foreign_table_stays_inside_the_buffers():
    """emulator only: boxes far outside the page, labels nobody has, counts beyond the table -- wrong numbers, no write outside"""
    page, text = ellipse_page(40, 50)
    with BACKENDS["emu"]() as dev:
        planes = Planes(dev, text, 6, None)
        planes.run(8, 0)
        table = np.array([[1, 5, -900, -900, 4000, 4000], [77, 5, 30, 40, 10, 5], [5, 1, 2 ** 31 - 1, 0, -2 ** 31, 7],
                          [2 ** 31 - 1, 0, 0, 0, 40, 50], [0, 0, 5, 5, 9, 9], [-3, 9, 39, 49, 41, 51]], np.int32)
        planes.table.raw[:table.nbytes] = torch.from_numpy(table.reshape(-1).view(np.uint8).copy())
        for count in (6, 2 ** 31 - 1, -5):
            planes.n.raw[:8] = torch.from_numpy(np.array([3, count], np.int32).view(np.uint8).copy())
            b = Balloons(dev, planes, page, 512)
            b.run(8, 255, 512)
            rows, rect, _, _ = b.get()
            exp = expected(text, 8, 0, None)
            ref = balloon_ref(page, exp["text"], exp["labels"], table, 6 if count > 0 else 0, 8, 255, 512)
            assert np.array_equal(rows[:len(ref[0])], ref[0]) and np.array_equal(rect[:len(ref[1])], ref[1])
            if count < 0:
                assert untouched(rows) and untouched(rect), "no row is served: nothing is written"
