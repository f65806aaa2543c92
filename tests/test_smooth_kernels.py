"""Smooth regions (csrc/smooth.hip, include/tsii_hip.h "K16: smooth regions") through the C ABI on the emulator (CPU suite) and, with
-m gpu, on the chip: a text region whose ring shows no step of more than ``tol`` between 4-neighbours is filled with the harmonic
continuation of its surroundings (``tsii_smooth_regions_classify``, ``tsii_harmonic_fill``, ``tsii_smooth_regions_apply``).

The semantics, restated.  ``R = min(n_regions[1], max_regions)``; for ``r < R``: ``C_r`` the pixels labelled ``table[r][0]`` whose text
byte is non-zero; ``Ring_r`` the page pixels that are not text on entry and lie within ``ring`` (Chebyshev) of a pixel of ``C_r``;
``n_r = |Ring_r|``; ``d_c(q)`` the largest ``|page[q][c] - page[q'][c]|`` over the non-text 4-neighbours of a non-text pixel;
``step_r[c] = max d_c`` over the ring; ``smooth_r`` iff ``n_r >= 1`` and every ``step_r[c] <= tol``; row ``r`` of ``smooth`` =
``(smooth_r, step_r, n_r)``.  ``x = byte / 255`` in fp32, ``valid = (text == 0)``.  Apply: ``painted`` =
``floor(clamp(filled, 0, 1) * 255 + 0.5)`` (fp32, product and sum rounded in turn) on the smooth ``C_r``, the page elsewhere; ``text`` = 0
on the smooth regions, else 1 where it was non-zero; ``mask`` = 255 where text was non-zero on entry; ``core_count`` = the text pixels of
the final plane per tile core.

The statistics are integers: every comparison is EQUALITY with a restatement of another structure than the kernels' (which walk windows
around the non-text pixels and take d from a staged block): per region, a max-pool dilation of the region's own pixels by ``2 ring + 1``,
minus the text; ``d`` from whole-array shifted differences masked by the non-text plane; maxima in Python integers.  Labels and tables
come from the fixed-point labelling of ``tests/test_text_regions.py``.  Every output carries a canary tail; the workspace is handed over
full of canary bytes, at exactly ``ws_bytes``.
"""
import functools

import numpy as np
import pytest
import torch

from tests.backends import BACKENDS, both_backends
from tests.test_flat_kernels import blocks_pattern, core_counts, untouched
from tests.test_pipeline_kernels import Buf, up
from tests.test_text_eraser import dilate_np
from tests.test_text_regions import HALO, IDS, TILE, Planes, expected, pattern
from text_segmentation_image_inpainting_amd import _lib
from text_segmentation_image_inpainting_amd.pipeline import tile_grid

PAGES = [(1, 1), (5, 217), (40, 50), (150, 217)]          # the last: more than one 64 x 32 block both ways
RINGS, TOLS = [1, 3, 8], [0, 8, 255]


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def local_step(page, text01):
    """int64 [h, w, 3]: d of every non-text pixel (0 on the text): shifted differences of the whole array, both ends non-text"""
    p, ok = page.astype(np.int64), ~text01
    d = np.zeros(p.shape, np.int64)
    dv = np.abs(p[1:] - p[:-1]) * (ok[1:] & ok[:-1])[..., None]
    d[1:] = np.maximum(d[1:], dv)
    d[:-1] = np.maximum(d[:-1], dv)
    dh = np.abs(p[:, 1:] - p[:, :-1]) * (ok[:, 1:] & ok[:, :-1])[..., None]
    d[:, 1:] = np.maximum(d[:, 1:], dh)
    d[:, :-1] = np.maximum(d[:, :-1], dh)
    return d


def smooth_ref(page, text, labels, table, n_rows, ring, tol):
    """-> the smooth rows [n_rows, 5]"""
    h, w = text.shape
    text01 = text != 0
    d, rows = local_step(page, text01), np.zeros((n_rows, 5), np.int32)
    for r in range(n_rows):
        y0, x0, y1, x1 = (int(v) for v in table[r][2:6])
        ya, xa, yb, xb = max(y0 - ring, 0), max(x0 - ring, 0), min(y1 + ring, h), min(x1 + ring, w)      # the ring lies in the grown box
        c = (labels[ya:yb, xa:xb] == table[r][0]) & text01[ya:yb, xa:xb]
        ringm = (dilate_np(c, 2 * ring + 1) != 0) & ~text01[ya:yb, xa:xb]
        n = int(ringm.sum())
        if n == 0:
            continue                                       # (0, 0, 0, 0, 0): never smooth
        step = [max(int(v) for v in d[ya:yb, xa:xb, ch][ringm]) for ch in range(3)]
        rows[r] = [int(all(s <= tol for s in step))] + step + [n]
    return rows


def round_byte(v):
    """floor(clamp(v, 0, 1) * 255 + 0.5): every fp32 operation rounded on its own"""
    c = np.clip(np.asarray(v, np.float32), np.float32(0), np.float32(1))
    return np.floor(c * np.float32(255) + np.float32(0.5)).astype(np.uint8)


def apply_ref(page, text, labels, table, rows, filled):
    """-> (painted, final text plane, mask)"""
    text01 = text != 0
    sel = np.zeros(text.shape, bool)
    for r in range(len(rows)):
        if rows[r][0]:
            sel |= (labels == table[r][0]) & text01
    painted = page.copy()
    painted[sel] = round_byte(filled[sel])
    return painted, (text01 & ~sel).astype(np.uint8), text01.astype(np.uint8) * 255


def stage_ref(page, text):
    return page.astype(np.float32) / np.float32(255), (text == 0).astype(np.float32)


# ---- pages -----------------------------------------------------------------------------------------------------------------------
def tri(v):
    """a triangle wave 0..255..0: a ramp that never wraps"""
    return np.abs((v % 510) - 255)


def quarters_page(h, w, tol, seed=3):
    """quarters of the page's width: a ramp of slope 1 per pixel (along x + y: smooth at tol 1, not at tol 0); a ramp of slope tol
    exactly; noise (never smooth below 255); one colour"""
    rng = np.random.default_rng(seed + h)
    yy, xx = np.mgrid[0:h, 0:w]
    quarter = np.minimum(xx * 4 // max(w, 1), 3)
    page = np.zeros((h, w, 3), np.int64)
    for c in range(3):
        ramps = [tri(xx + yy + 40 * c), tri(xx * tol + 17 * c), rng.integers(0, 256, size=(h, w)), np.full((h, w), 60 + 50 * c)]
        page[..., c] = np.choose(quarter, ramps)
    return page.astype(np.uint8)


def make_filled(rng, h, w, keep):
    """fp32 [h, w, 3] of the test's own: values below 0, above 1 and at exact .5 / 255 boundaries; NaN wherever ``keep`` is False"""
    f = rng.uniform(-0.3, 1.3, size=(h, w, 3)).astype(np.float32)
    k = rng.integers(0, 255, size=(h, w, 3))
    bound = ((k.astype(np.float64) + 0.5) / 255.0).astype(np.float32)
    which = rng.integers(0, 4, size=(h, w, 3))
    f = np.where(which == 0, bound, np.where(which == 1, np.nextafter(bound, np.float32(0)), f)).astype(np.float32)
    f[~keep] = np.nan
    return f


def text_of(name, h, w):
    return blocks_pattern(h, w) if name == "blocks" else pattern(name, h, w)


@functools.lru_cache(maxsize=None)
def regions_of(name, h, w, connectivity):
    text = text_of(name, h, w)
    return text, expected(text, connectivity, 0, tile_grid(h, w, TILE, HALO))


@functools.lru_cache(maxsize=None)
def case(name, h, w, connectivity, ring, tol, max_regions=None):
    """(page, text, max_regions, rows, filled, (painted, rest, mask)): computed once; callers do not modify it"""
    text, exp = regions_of(name, h, w, connectivity)
    page = quarters_page(h, w, tol)
    max_regions = exp["n"][1] + 3 if max_regions is None else max_regions
    n_rows = min(exp["n"][1], max_regions)
    rows = smooth_ref(page, exp["text"], exp["labels"], exp["table"], n_rows, ring, tol)
    keep = np.zeros((h, w), bool)
    for r in range(n_rows):
        if rows[r][0]:
            keep |= exp["labels"] == exp["table"][r][0]
    filled = make_filled(np.random.default_rng(h * w + ring), h, w, keep)
    return page, text, max_regions, rows, filled, apply_ref(page, exp["text"], exp["labels"], exp["table"], rows, filled)


# ---- the kernels -----------------------------------------------------------------------------------------------------------------
class Smooth:
    """the extra buffers of the two tsii_smooth_regions calls behind a ``Planes`` of tests/test_text_regions.py"""

    def __init__(self, dev, planes, page, ws=None):
        self.p, n = planes, planes.h * planes.w
        self.dev, self.page = dev, up(dev, page)
        self.painted, self.mask = Buf(dev, 3 * n, torch.uint8), Buf(dev, n, torch.uint8)
        self.smooth, self.core = Buf(dev, 5 * planes.max_regions, torch.int32), Buf(dev, planes.g.count, torch.int32)
        self.x, self.valid = Buf(dev, 3 * n, torch.float32), Buf(dev, n, torch.float32)
        nbytes = _lib.lib().tsii_smooth_regions_ws_bytes(planes.h, planes.w, planes.max_regions)
        assert nbytes == 16 * planes.max_regions
        self.ws = Buf(dev, nbytes // 4, torch.int32) if ws is None else ws
        self.filled = None

    def classify(self, ring, tol, **bad):
        p = self.p
        a = dict(page=_lib.ptr(self.page), text=p.text.ptr, labels=p.labels.ptr, h=p.h, w=p.w, table=p.table.ptr, n=p.n.ptr,
                 max_regions=p.max_regions, smooth=self.smooth.ptr, x=self.x.ptr, valid=self.valid.ptr, ws=self.ws.ptr)
        a.update(bad)
        _lib.call("tsii_smooth_regions_classify", a["page"], a["text"], a["labels"], a["h"], a["w"], a["table"], a["n"], a["max_regions"], ring,
                  tol, a["smooth"], a["x"], a["valid"], a["ws"], _lib.stream())

    def harmonic(self, sweeps):
        """tsii_harmonic_fill on the staged operands -> self.filled"""
        p = self.p
        n = p.h * p.w
        self.filled = torch.full((3 * n,), float("nan"), dtype=torch.float32, device=self.dev)
        ws = torch.empty(_lib.lib().tsii_harmonic_fill_ws_bytes(1, p.h, p.w) // 4 + 4, dtype=torch.float32, device=self.dev)
        _lib.call("tsii_harmonic_fill", self.x.ptr, self.valid.ptr, 1, p.h, p.w, sweeps, _lib.ptr(self.filled), _lib.ptr(ws), _lib.stream())

    def apply(self, filled=None, counts=True, mask=True, tile=TILE, halo=HALO, **bad):
        p = self.p
        if filled is not None:
            self.filled = up(self.dev, filled)
        a = dict(page=_lib.ptr(self.page), text=p.text.ptr, labels=p.labels.ptr, h=p.h, w=p.w, table=p.table.ptr, n=p.n.ptr,
                 max_regions=p.max_regions, smooth=self.smooth.ptr, filled_ptr=_lib.ptr(self.filled), painted=self.painted.ptr)
        a.update(bad)
        _lib.call("tsii_smooth_regions_apply", a["page"], a["text"], a["labels"], a["h"], a["w"], a["table"], a["n"], a["max_regions"],
                  a["smooth"], a["filled_ptr"], tile, halo, self.core.ptr if counts else None, a["painted"], self.mask.ptr if mask else None,
                  _lib.stream())

    def staged(self):
        p = self.p
        self.ws.get()
        return self.smooth.get().reshape(-1, 5), self.x.get().reshape(p.h, p.w, 3), self.valid.get().reshape(p.h, p.w)

    def applied(self):
        p = self.p
        return self.painted.get().reshape(p.h, p.w, 3), p.text.get().reshape(p.h, p.w), self.mask.get().reshape(p.h, p.w), self.core.get()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def check_staged(got, rows, page, text):
    got_rows, x, valid = got
    assert np.array_equal(got_rows[:len(rows)], rows), (got_rows[:len(rows)], rows)
    assert untouched(got_rows[len(rows):]), "rows of smooth behind R must not be touched"
    ref_x, ref_valid = stage_ref(page, text)
    assert same_bits(x, ref_x) and same_bits(valid, ref_valid)


def check_applied(got, ref, g, counts=True, mask=True):
    painted, text, got_mask, core = got
    ref_painted, ref_text, ref_mask = ref
    assert np.array_equal(text, ref_text), int((text != ref_text).sum())
    assert np.array_equal(painted, ref_painted), int((painted != ref_painted).sum())
    assert np.array_equal(got_mask, ref_mask) if mask else untouched(got_mask)
    assert np.array_equal(core, core_counts(ref_text, g)) if counts else untouched(core)


def run_page(backend, page, text, ring, tol, rows, filled, ref, max_regions, connectivity=8, prepare=None, **kw):
    """classify (compared), then apply on the test's own ``filled`` (compared); labels, table, counts and the page are read only"""
    h, w = text.shape
    g = tile_grid(h, w, TILE, HALO)
    with BACKENDS[backend]() as dev:
        planes = Planes(dev, text, max_regions, g)
        planes.run(connectivity, 0)
        if prepare is not None:
            prepare(planes)
        before = planes.get()
        sm = Smooth(dev, planes, page)
        sm.classify(ring, tol)
        staged = sm.staged()
        assert np.array_equal(planes.get()["text"], before["text"]), "classify reads the text plane only"
        assert all(untouched(a) for a in (sm.painted.get(), sm.mask.get(), sm.core.get()))
        sm.apply(filled, **kw)
        applied = sm.applied()
        after = planes.get()
        page_after = sm.page.cpu().numpy()
    for key in ("labels", "table", "n"):
        assert np.array_equal(np.asarray(before[key]), np.asarray(after[key])), f"{key} is read only"
    assert np.array_equal(page_after, page), "the page is read only"
    check_staged(staged, rows, page, before["text"])
    check_applied(applied, ref, g, **kw)


def run_case(backend, name, hw, connectivity, ring, tol, max_regions=None, **kw):
    page, text, max_regions, rows, filled, ref = case(name, *hw, connectivity, ring, tol, max_regions)
    run_page(backend, page, text, ring, tol, rows, filled, ref, max_regions, connectivity, **kw)
    return rows, ref


def run_custom(backend, page, text, ring, tol, max_regions=8, prepare_ref=None, prepare=None):
    """one pair of calls on a hand-made page -> the rows (already compared with the device's)"""
    h, w = text.shape
    exp = expected(text, 8, 0, tile_grid(h, w, TILE, HALO))
    plane = exp["text"] if prepare_ref is None else prepare_ref(exp["text"].copy())
    n_rows = min(exp["n"][1], max_regions)
    rows = smooth_ref(page, plane, exp["labels"], exp["table"], n_rows, ring, tol)
    keep = np.zeros((h, w), bool)
    for r in range(n_rows):
        if rows[r][0]:
            keep |= (exp["labels"] == exp["table"][r][0]) & (plane != 0)
    filled = make_filled(np.random.default_rng(5), h, w, keep)
    ref = apply_ref(page, plane, exp["labels"], exp["table"], rows, filled)
    run_page(backend, page, text, ring, tol, rows, filled, ref, max_regions, prepare=prepare)
    return rows, ref


@both_backends
@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("ring", RINGS)
@pytest.mark.parametrize("hw", PAGES, **IDS)
def test_blocks(backend, hw, ring, tol):
    """components across the lines x = 63 / 64 and y = 31 / 32, in all four corners and against all four page edges, on the quarters page"""
    rows, (painted, rest, mask) = run_case(backend, "blocks", hw, 8, ring, tol)
    if tol == 255:
        assert bool((rows[:, 0] == (rows[:, 4] >= 1)).all()), "full tolerance: everything with a ring is smooth"
        assert not rest.any() or hw == (1, 1)
    if hw == (150, 217):
        assert len(rows) == 15 and (tol == 255 or 0 < rows[:, 0].sum() < 15), rows[:, 0]
        assert mask[31, 63] == mask[32, 64] == 255 and mask[0, 0] == mask[149, 216] == mask[0, 216] == mask[149, 0] == 255
        if tol == 0:                                       # the slope-1 ramp steps by 1, the tol-slope ramp is one colour per channel
            assert rows[0].tolist()[:4] == [0, 1, 1, 1]


@both_backends
@pytest.mark.parametrize("ring,tol", [(1, 0), (3, 8), (8, 255), (8, 60)])
@pytest.mark.parametrize("name,connectivity", [("noise0.3", 4), ("noise0.45", 8)])
@pytest.mark.parametrize("hw", PAGES, **IDS)
def test_noise(backend, hw, name, connectivity, ring, tol):
    """thousands of small regions: windows with many distinct rows, more rows per block than its LDS table holds"""
    rows = run_case(backend, name, hw, connectivity, ring, tol)[0]
    if hw == (150, 217) and connectivity == 4:
        assert len(rows) > 2000


@both_backends
@pytest.mark.parametrize("hw", PAGES, **IDS)
def test_no_ring(backend, hw):
    """a component that fills the whole page has n = 0 and is not smooth; a page without text has no row at all"""
    rows, (painted, rest, mask) = run_case(backend, "full", hw, 8, 3, 255)
    assert rows.tolist() == [[0, 0, 0, 0, 0]] and bool(rest.all()) and bool((mask == 255).all())
    rows, (painted, rest, mask) = run_case(backend, "empty", hw, 8, 3, 255)
    assert len(rows) == 0 and not mask.any()


def ramp_page(h, w, slopes):
    xx = np.mgrid[0:h, 0:w][1]
    return np.stack([tri(xx * s + 30) for s in slopes], axis=-1).astype(np.uint8)


@both_backends
@pytest.mark.parametrize("channel", [0, 1, 2])
def test_slope_boundary(backend, channel):
    """a ramp of slope tol exactly is smooth, one of tol + 1 is not; the excess in one channel only.  A ramp of slope 1: tol 1, not tol 0"""
    text = np.zeros((40, 50), np.uint8)
    text[20:24, 20:30] = 1
    for excess, is_smooth in ((0, 1), (1, 0)):
        slopes = [8, 8, 8]
        slopes[channel] += excess
        rows, (painted, rest, mask) = run_custom(backend, ramp_page(40, 50, slopes), text, 3, 8)
        assert rows[0].tolist() == [is_smooth] + slopes + [10 * 16 - 40]
        assert bool(rest.any()) != bool(is_smooth)
    for tol, is_smooth in ((1, 1), (0, 0)):
        assert run_custom(backend, ramp_page(40, 50, [1, 1, 1]), text, 3, tol)[0][0].tolist() == [is_smooth, 1, 1, 1, 120]


@both_backends
def test_hard_edges(backend):
    """a hard edge that crosses the ring on one side only counts; one that runs just outside the ring + 1 reach does not"""
    text = np.zeros((40, 50), np.uint8)
    text[20:24, 20:30] = 1                                 # ring 3: rows 17..26, columns 17..32
    page = np.full((40, 50, 3), 100, np.uint8)
    page[:, 32:, 1] = 160                                  # the step lies between columns 31 and 32: inside the ring, on its right side only
    assert run_custom(backend, page, text, 3, 8)[0][0].tolist() == [0, 0, 60, 0, 120]
    page = np.full((40, 50, 3), 100, np.uint8)
    page[:, 33:, 1] = 160                                  # column 32 is the ring's last and sees column 33: still counts
    assert run_custom(backend, page, text, 3, 8)[0][0].tolist() == [0, 0, 60, 0, 120]
    page = np.full((40, 50, 3), 100, np.uint8)
    page[:, 34:, 1] = 160                                  # between columns 33 and 34: no ring pixel has a neighbour beyond it
    page[:16] = 7                                          # and above: the step between rows 15 and 16 is not seen from row 17
    assert run_custom(backend, page, text, 3, 8)[0][0].tolist() == [1, 0, 0, 0, 120]


@both_backends
def test_close_neighbours(backend):
    """two 5 x 5 squares 2 pixels apart, ring 3, black ink on white: the pixels between them count for both rings, the neighbour's text
    pixels are in no ring and no d uses them (step 0 although the ink differs from the paper by 255)"""
    page = np.full((40, 50, 3), 255, np.uint8)
    text = np.zeros((40, 50), np.uint8)
    text[10:15, 10:15] = text[10:15, 17:22] = 1
    page[text != 0] = 0
    rows = run_custom(backend, page, text, 3, 0)[0]
    assert rows.tolist() == [[1, 0, 0, 0, 11 * 11 - 25 - 5]] * 2
    page[12, 16] = 250                                     # a speck between them: in both rings
    assert run_custom(backend, page, text, 3, 4)[0].tolist() == [[0, 5, 5, 5, 91]] * 2


@both_backends
def test_behind_flat(backend):
    """a region whose text bytes were cleared while its label stays, as tsii_flat_regions leaves it: C_r is empty, its row is zeros, its
    pixels are valid context, in the rings of its neighbours, and stay as the page has them"""
    page = ramp_page(40, 50, [2, 3, 4])
    text = np.zeros((40, 50), np.uint8)
    text[10:15, 10:15] = text[10:15, 17:22] = 1

    def clear_ref(plane):
        plane[10:15, 10:15] = 0
        return plane

    def clear(planes):
        t = planes.text.raw[:40 * 50].view(40, 50)
        t[10:15, 10:15] = 0

    rows, (painted, rest, mask) = run_custom(backend, page, text, 3, 8, prepare_ref=clear_ref, prepare=clear)
    assert rows.tolist() == [[0, 0, 0, 0, 0], [1, 2, 3, 4, 11 * 11 - 25]]
    assert not rest.any() and mask.sum() == 255 * 25 and np.array_equal(painted[10:15, 10:15], page[10:15, 10:15])


@both_backends
def test_truncation(backend):
    """max_regions = 2 with four components: rows 2 and 3 stay text, their smooth rows keep the canary (checked in check_staged)"""
    text = np.zeros((40, 50), np.uint8)
    for k in range(4):
        text[5 + 6 * k:9 + 6 * k, 10:20] = 1               # 4 rows each, 2 rows apart
    page = ramp_page(40, 50, [1, 2, 3])
    rows, (painted, rest, mask) = run_custom(backend, page, text, 3, 3, max_regions=2)
    assert rows[:, 0].tolist() == [1, 1] and not rest[:17].any() and bool(rest[17:21, 10:20].all()) and bool(rest[23:27, 10:20].all())
    assert mask.sum() == 255 * 160 and np.array_equal(painted[17:], page[17:])
    # a region beyond the table is text to its neighbour's ring as well
    assert rows[:, 4].tolist() == [10 * 16 - 40 - 10, 10 * 16 - 40 - 20]


@both_backends
@pytest.mark.parametrize("hw", PAGES[2:], **IDS)
def test_without_core_counts_and_without_mask(backend, hw):
    run_case(backend, "blocks", hw, 8, 3, 8, counts=False)
    run_case(backend, "blocks", hw, 8, 3, 8, mask=False)


@both_backends
def test_end_to_end_and_one_workspace_for_three_calls(backend):
    """classify, tsii_harmonic_fill, apply == tsii_harmonic_fill run by the test on the restated x and valid, rounded by the rule; the same
    from one workspace (of the classify call) reused over three calls"""
    a, b = case("blocks", 150, 217, 8, 3, 8, 512), case("noise0.45", 150, 217, 8, 8, 60, 512)
    g = tile_grid(150, 217, TILE, HALO)
    with BACKENDS[backend]() as dev:
        ws, results, refs = None, [], []
        for (page, text, max_regions, rows, _, _), (ring, tol) in zip((a, b, a), ((3, 8), (8, 60), (3, 8))):
            planes = Planes(dev, text, max_regions, g)
            planes.run(8, 0)
            before = planes.get()
            sm = Smooth(dev, planes, page, ws=ws)
            ws = sm.ws
            sm.classify(ring, tol)
            sm.harmonic(8)
            sm.apply()
            results.append((sm.staged(), sm.applied()))
            # the test's own solver call on the restated operands
            x, valid = stage_ref(page, before["text"])
            xd, vd = up(dev, x), up(dev, valid)
            out = torch.empty_like(xd)
            hws = torch.empty(_lib.lib().tsii_harmonic_fill_ws_bytes(1, 150, 217) // 4 + 4, dtype=torch.float32, device=dev)
            _lib.call("tsii_harmonic_fill", _lib.ptr(xd), _lib.ptr(vd), 1, 150, 217, 8, _lib.ptr(out), _lib.ptr(hws), _lib.stream())
            refs.append(apply_ref(page, before["text"], before["labels"], before["table"], rows, out.cpu().numpy()))
    for (staged, applied), c, ref in zip(results, (a, b, a), refs):
        assert np.array_equal(staged[0][:len(c[3])], c[3])
        check_applied(applied, ref, g)
    assert results[0][1][1].sum() < a[5][2].sum() // 255, "some region of the first page is smooth"
    assert all(np.array_equal(p, q) for p, q in zip(results[0][1], results[2][1]))


@both_backends
def test_refusals(backend):
    page, text, max_regions, _, filled, _ = case("blocks", 40, 50, 8, 3, 8)
    lib = _lib.lib
    with BACKENDS[backend]() as dev:
        assert lib().tsii_smooth_regions_ws_bytes(26755, 26755, 1) == 0 and lib().tsii_smooth_regions_ws_bytes(0, 5, 1) == 0
        assert lib().tsii_smooth_regions_ws_bytes(5, 0, 1) == 0 and lib().tsii_smooth_regions_ws_bytes(5, 5, 0) == 0
        assert lib().tsii_smooth_regions_ws_bytes(26754, 26754, 1) == 16
        planes = Planes(dev, text, max_regions, tile_grid(40, 50, TILE, HALO))
        planes.run(8, 0)
        before = planes.get()
        sm = Smooth(dev, planes, page)
        sm.filled = up(dev, np.nan_to_num(filled))
        for ring, tol in ((0, 8), (9, 8), (3, -1), (3, 256)):
            with pytest.raises(RuntimeError, match=r"tsii_smooth_regions_classify failed \(-?[1-9]\d*\): .*(ring|tol)"):
                sm.classify(ring, tol)
        common = [dict(h=0), dict(w=0), dict(h=26755, w=26755), dict(max_regions=0), dict(labels=None), dict(page=None), dict(text=None),
                  dict(table=None), dict(n=None), dict(smooth=None)]
        for bad in common + [dict(x=None), dict(valid=None), dict(ws=None)]:
            with pytest.raises(RuntimeError, match=r"tsii_smooth_regions_classify failed \(-?[1-9]\d*\): "):
                sm.classify(3, 8, **bad)
        for bad in common + [dict(filled_ptr=None), dict(painted=None), dict(painted=_lib.ptr(sm.page))]:
            with pytest.raises(RuntimeError, match=r"tsii_smooth_regions_apply failed \(-?[1-9]\d*\): "):
                sm.apply(**bad)
        with pytest.raises(RuntimeError, match="geometry"):
            sm.apply(tile=48, halo=4)
        with pytest.raises(RuntimeError, match="geometry"):
            sm.apply(tile=64, halo=32)
        outputs = [sm.smooth.get(), sm.x.get(), sm.valid.get(), sm.painted.get(), sm.mask.get(), sm.core.get(), sm.ws.get()]
        after = planes.get()
    assert np.array_equal(after["text"], before["text"]), "a refused call must not touch the text plane"
    assert all(untouched(a) for a in outputs)
    for key in ("labels", "table", "n"):
        assert np.array_equal(np.asarray(before[key]), np.asarray(after[key]))


def test_foreign_table_stays_inside_the_buffers():
    """EMULATOR ONLY: a count that is out of range and labels the table does not know give wrong bytes but leave every canary intact"""
    page, text, _, _, filled, _ = case("noise0.45", 40, 50, 8, 3, 8)
    big, max_regions = 2 ** 31 - 1, 16
    tables = [[[k * 7 - 20, 1, -big, -big, big, big] for k in range(16)], [[5, 1, 0, 0, 1, 1]] * 16, [[big - k, 1, 0, 0, 1, 1] for k in range(16)]]
    with BACKENDS["emu"]() as dev:
        for table in tables:
            for count in (big, -3, 16, 5):
                planes = Planes(dev, text, max_regions, tile_grid(40, 50, TILE, HALO))
                planes.run(8, 0)
                planes.table.raw[:4 * 6 * max_regions] = torch.from_numpy(np.array(table, np.int32).reshape(-1).view(np.uint8).copy())
                planes.n.raw[:8] = torch.from_numpy(np.array([count, count], np.int32).view(np.uint8).copy())
                sm = Smooth(dev, planes, page)
                sm.classify(8, 255)
                sm.staged()
                sm.apply(np.nan_to_num(filled))
                painted, out, mask, core = sm.applied()
                planes.get()
                assert set(np.unique(out)) <= {0, 1} and int(core.sum()) == int(out.sum()) and np.array_equal(mask, (text != 0) * 255)
