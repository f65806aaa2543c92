"""Text regions on the device: connected components of a text plane, their areas and boxes, and a minimum-area filter.

The counterpart of the reference demo's ``draw_bounding_box(origin_np, mask_np, 500)``: label the mask, drop the specks, say where the
text is.  One entry point, ``tsii_text_regions`` (``csrc/regions.hip``; semantics: ``include/tsii_hip.h``, "K10: text regions"); all
integer, so the result has the same bits on every run.  ``text_regions`` is the stand-alone form; ``TextEraser`` runs the same kernels
in place on its text plane between the mask and the tile selection (``pipeline.py``).

``fill_region_hulls`` is the demo's next step, ``cv2.convexHull`` + ``cv2.drawContours(..., -1)``: the convex hull of every kept region
filled into the plane (``tsii_region_hulls``, ``csrc/hull.hip``; "K12: region hulls"), behind the same labelling.

``flat_fill_regions`` is the reference README's middle step, "use the generated mask to white out words", for text on one flat colour:
a region whose surrounding ring of page pixels is uniform within a tolerance is painted with the ring's mean colour and leaves the
plane (``tsii_flat_regions``, ``csrc/flat.hip``; "K13: flat regions"); what is left is the text an inpainting net has to see.

``smooth_fill_regions`` is the route between that and a net, for text on a smooth background (a gradient, a soft shadow, a sky): a region
whose ring shows no step of more than a tolerance between neighbouring pixels is filled with the harmonic continuation of its
surroundings at page level (``tsii_smooth_regions_classify`` / ``tsii_smooth_regions_apply``, ``csrc/smooth.hip``; "K16: smooth regions",
around the ``tsii_harmonic_fill`` of ``fill.py``) and leaves the plane.

``tone_fill_regions`` is the third route without a net, for text on a periodic pattern (screentone, stripes, a dot lattice): a region
whose ring repeats under one integer shift is filled by copying the pixel a whole number of periods away (``tsii_tone_regions``,
``csrc/tone.hip``; "K17: tone regions") and leaves the plane.

``text_blocks`` groups the regions into blocks of lettering: two regions belong together when some pixel of one is within ``gap`` pixels
(Chebyshev distance) of some pixel of the other, and so on through their neighbours (``tsii_text_blocks``, ``csrc/blocks.hip``; "K15:
text blocks").  The block labels and the block table have the form of the regions' own, so the hulls, the flat stage and the window
planner work per block behind it.

``seeded_regions`` is a hysteresis threshold: the plane was cut at a low probability; a region (with ``gap``: a block) stays only where at
least ``min_seeds`` of its pixels are set in a second plane, cut at a high one (``tsii_region_seeds``, ``csrc/seeds.hip``; "K19: seeded
regions").  The dropped regions leave the plane, the labels and the table on the device, before the read-back.

``region_geometry`` gives every region (with ``gap``: every block) the polygon of its convex hull and its minimum-area enclosing rectangle,
``cv2.convexHull`` and ``cv2.minAreaRect`` in integers (``tsii_region_geometry``, ``csrc/hull.hip`` behind the hull's own kernels; "K22:
region geometry"): the oriented box a translation is typeset into, and the text angle.

``region_crops`` cuts every such rectangle out of the page, deskewed and scaled into a fixed slot, and leaves the batch on the device
(``tsii_region_crops``, ``csrc/crops.hip``; "K23: region crops"): the picture an OCR net or a reviewer starts from.

``paste_crops`` is the way back: a batch of RGBA pictures, one per slot, is laid onto a page along the rectangles the crops' ``info`` names,
antialiased and alpha-blended in row order (``tsii_region_paste``, ``csrc/paste.hip``; "K24: region paste"): the translated lettering on the
cleaned page.

``region_balloons`` says where a translation has room: for every region (with ``gap``: every block) the speech balloon around it -- the
flood fill from the lettering over the colour of its ring --, its area and box, whether it is closed, and the largest upright rectangle
inside it around the block's centre, as a ``rect`` row ``region_crops`` and ``paste_crops`` take (``tsii_region_balloons``,
``csrc/balloon.hip``; "K25: region balloons").
"""
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, ops
from ._lib import call, ptr
from .fill import _harmonic_fill, check_sweeps


class RegionHulls(NamedTuple):
    """``filled``: uint8 ``[H, W]`` of 0 / 255, the text plane with the convex hull of every kept region filled in.  ``regions``: the
    ``TextRegions`` of the input.  ``hull_area``: numpy int32 ``[n]``, the pixels of each table row's hull."""
    filled: object
    regions: "TextRegions"
    hull_area: np.ndarray


class FlatFill(NamedTuple):
    """``painted``: uint8 ``[H, W, 3]``, the page with every flat region in its ring's mean colour.  ``rest``: uint8 ``[H, W]`` of
    0 / 255, the text that is left for a net.  ``regions``: the ``TextRegions`` of the input.  Per table row: ``is_flat`` (numpy bool
    ``[n]``), ``colour`` (uint8 ``[n, 3]``, the rounded mean of the ring; 0 without a ring) and ``ring_pixels`` (int32 ``[n]``)."""
    painted: object
    rest: object
    regions: "TextRegions"
    is_flat: np.ndarray
    colour: np.ndarray
    ring_pixels: np.ndarray


class SmoothFill(NamedTuple):
    """``painted``: uint8 ``[H, W, 3]``, the page with every smooth region filled harmonically.  ``text``: uint8 ``[H, W]`` of 0 / 255,
    the text that is left for a net.  ``table``: numpy int32 ``[n, 6]``, the region table (``TextRegions.table``).  Per table row:
    ``is_smooth`` (numpy bool ``[n]``), ``step`` (uint8 ``[n, 3]``, the largest difference between 4-neighbours in the ring, per channel;
    0 without a ring) and ``ring_pixels`` (int32 ``[n]``)."""
    painted: object
    text: object
    table: np.ndarray
    is_smooth: np.ndarray
    step: np.ndarray
    ring_pixels: np.ndarray


class ToneFill(NamedTuple):
    """``painted``: uint8 ``[H, W, 3]``, the page with every tone region filled from one period away.  ``text``: uint8 ``[H, W]`` of 0 / 255,
    the text that is left for a net.  ``table``: numpy int32 ``[n, 6]``, the region table (``TextRegions.table``).  Per table row:
    ``is_tone`` (numpy bool ``[n]``), ``shift`` (int32 ``[n, 2]``: ``dy, dx`` of the ring's period, 0 0 without one), ``err`` (int32
    ``[n]``: the largest difference under that shift), ``step`` (int32 ``[n]``: the largest difference under a shift of one pixel) and
    ``ring_pixels`` (int32 ``[n]``)."""
    painted: object
    text: object
    table: np.ndarray
    is_tone: np.ndarray
    shift: np.ndarray
    err: np.ndarray
    step: np.ndarray
    ring_pixels: np.ndarray


class TextRegions(NamedTuple):
    """``labels``: int32 ``[H, W]``, 0 = background or a dropped region, else ``1 + min(y * W + x)`` over the region's pixels.
    ``table``: numpy int32 ``[n, 6]``, one row ``(label, area, y0, x0, y1, x1)`` per kept region (``y1``, ``x1`` exclusive) in raster
    order of the regions' first pixels, ``n = min(kept, max_regions)``.  ``found`` / ``kept``: regions before / after the filter.
    ``truncated``: ``kept > max_regions``, the table holds the first ``max_regions`` rows only."""
    labels: object
    table: np.ndarray
    found: int
    kept: int
    truncated: bool


class TextBlocks(NamedTuple):
    """``mask``: uint8 ``[H, W]`` of 0 / 255, the text of the kept blocks.  ``labels``: int32 ``[H, W]``, 0 = background or a dropped
    block, else ``1 + min(y * W + x)`` over the block's pixels.  ``table``: numpy int32 ``[n, 6]``, one row ``(label, area, y0, x0, y1,
    x1)`` per kept block in raster order of the blocks' first pixels, ``n = min(kept, max_regions)``; ``members``: numpy int32 ``[n]``,
    the connected regions in each.  ``found`` / ``kept``: blocks before / after the area filter (``kept > len(table)``: the table is
    cut at ``max_regions``).  ``components``: the connected regions of the plane."""
    mask: object
    labels: object
    table: np.ndarray
    members: np.ndarray
    found: int
    kept: int
    components: int


class SeededRegions(NamedTuple):
    """``mask``: uint8 ``[H, W]`` of 0 / 255, the text of the regions that hold a seed.  ``labels`` / ``table`` / ``found`` / ``truncated``: as
    in ``TextRegions`` (with ``gap``: ``TextBlocks``), of those regions only; ``kept``: the regions left after both filters.  ``seeds``: numpy
    int32 ``[n]``, the seed pixels of each table row.  ``dropped`` / ``dropped_pixels``: the regions that held fewer than ``min_seeds`` seeds
    and their summed area.  ``members``: numpy int32 ``[n]`` with ``gap``, else None."""
    mask: object
    labels: object
    table: np.ndarray
    seeds: np.ndarray
    found: int
    kept: int
    dropped: int
    dropped_pixels: int
    truncated: bool
    members: np.ndarray = None


class RegionGeometry(NamedTuple):
    """``regions``: the ``TextRegions`` of the input (with ``gap``: its ``TextBlocks``); per table row ``r``: ``n_vertices`` (numpy int32
    ``[n]``: the vertices of the region's convex hull, the true count), ``vertices`` (int32 ``[n, max_vertices, 2]``: ``(y, x)`` of the
    first ``max_vertices`` of them, from the top-left one clockwise on the screen; the slots behind a row's count are 0) and ``rect`` (int64
    ``[n, 8]``: ``k, dy, dx, lo_d, hi_d, lo_n, hi_n, D`` of the minimum-area enclosing rectangle, "K22" of ``include/tsii_hip.h``: the hull
    edge ``k`` it lies along, the edge's direction ``d = (dy, dx)``, the extreme dot products of the hull with ``d`` and with the normal ``n =
    (-dx, dy)``, and ``D = |d|^2``).  All integers as the device left them; the helpers below are plain numpy on them."""
    regions: object
    n_vertices: np.ndarray
    vertices: np.ndarray
    rect: np.ndarray

    def polygon(self, r):
        """int32 ``[k, 2]``: the ``(y, x)`` hull vertices of row ``r`` in order, ``k = min(n_vertices[r], max_vertices)``"""
        return self.vertices[r, :min(int(self.n_vertices[r]), self.vertices.shape[1])].copy()

    def _axes(self, r, pad):
        _, dy, dx, lo_d, hi_d, lo_n, hi_n, dd = (float(v) for v in self.rect[r])
        grow = 0.5 * (abs(dy) + abs(dx)) if pad else 0.0        # the support of a pixel's square along d and along n, in their units
        return dy, dx, lo_d - grow, hi_d + grow, lo_n - grow, hi_n + grow, dd

    def box_points(self, r, pad=False):
        """float64 ``[4, 2]``: the ``(y, x)`` corners of row ``r``'s rectangle, from ``rect`` alone: ``(a d + b n) / D`` for ``(a, b)`` =
        (lo_d, lo_n), (hi_d, lo_n), (hi_d, hi_n), (lo_d, hi_n).  It encloses the pixel CENTRES; ``pad=True`` grows it so that it covers the
        pixels' unit squares."""
        dy, dx, lo_d, hi_d, lo_n, hi_n, dd = self._axes(r, pad)
        d, n = np.array([dy, dx]), np.array([-dx, dy])
        return np.stack([(a * d + b * n) / dd for a, b in ((lo_d, lo_n), (hi_d, lo_n), (hi_d, hi_n), (lo_d, hi_n))])

    def size(self, r, pad=False):
        """(along, across): the rectangle's side along its edge ``d`` and the one across it, in pixels; their product is the area"""
        _, _, lo_d, hi_d, lo_n, hi_n, dd = self._axes(r, pad)
        return (hi_d - lo_d) / np.sqrt(dd), (hi_n - lo_n) / np.sqrt(dd)

    def angle(self, r):
        """degrees from the x axis to the rectangle's LONGER side (the edge's direction where both are equal), in ``(-90, 90]``; positive
        turns towards +y, clockwise on a screen whose y points down"""
        _, dy, dx, lo_d, hi_d, lo_n, hi_n, _ = (int(v) for v in self.rect[r])
        if hi_n - lo_n > hi_d - lo_d:
            dy, dx = dx, -dy                                    # the normal's line
        a = float(np.degrees(np.arctan2(dy, dx)))
        return a - 180.0 if a > 90.0 else a + 180.0 if a <= -90.0 else a


class RegionCrops(NamedTuple):
    """``crops``: uint8 ``[n, ch, cw, 3]``, slot ``r`` the picture of table row ``r``: the row's padded minimum-area rectangle cut out of the
    page, deskewed and scaled to ``uh x uw`` pixels in the slot's top-left corner, the rest ``fill``.  ``info``: numpy int32 ``[n, 10]``,
    ``(uh, uw, f, s, O_y, O_x, SU_y, SU_x, SV_y, SV_x)`` per row ("K23" of ``include/tsii_hip.h``): the frame ``f``, the supersampling
    factor ``s``, and in units of 2^-12 page pixel the rectangle's corner ``O`` and its sides ``SU`` (the crop's x axis) and ``SV`` (its y
    axis).  A row without pixels has ``info`` 0 and an all-``fill`` slot.  The helpers are plain numpy on ``info``."""
    crops: object
    info: np.ndarray

    def crop(self, r):
        """the ``[uh, uw, 3]`` view of slot ``r``"""
        return self.crops[r, :int(self.info[r, 0]), :int(self.info[r, 1])]

    def quad(self, r):
        """float64 ``[4, 2]``: the page ``(y, x)`` of the crop's corners, top-left, top-right, bottom-right, bottom-left"""
        o, su, sv = (self.info[r, k:k + 2].astype(np.float64) / 4096.0 for k in (4, 6, 8))
        return np.stack([o, o + su, o + su + sv, o + sv])

    def to_page(self, r, i, j):
        """the page ``(y, x)`` of the centre of crop pixel ``(i, j)`` (fractions allowed: ``(-0.5, -0.5)`` is the top-left corner)"""
        uh, uw = int(self.info[r, 0]), int(self.info[r, 1])
        o, su, sv = (self.info[r, k:k + 2].astype(np.float64) / 4096.0 for k in (4, 6, 8))
        return o + su * ((2.0 * j + 1.0) / (2.0 * uw)) + sv * ((2.0 * i + 1.0) / (2.0 * uh))

    def scale(self, r):
        """(along u, along v): page pixels per crop pixel along the crop's x and y axes; below 1 where the block was magnified"""
        uh, uw = int(self.info[r, 0]), int(self.info[r, 1])
        return float(np.hypot(*self.info[r, 6:8].astype(np.float64))) / 4096.0 / uw, float(np.hypot(*self.info[r, 8:10].astype(np.float64))) / 4096.0 / uh

    def paste(self, page_u8, slots, **kw):
        """``paste_crops(page_u8, slots, self.info, **kw)``: pictures drawn into these slots, laid back where the crops came from"""
        return paste_crops(page_u8, slots, self.info, **kw)


class RegionBalloons(NamedTuple):
    """The speech balloon of every table row ("K25" of ``include/tsii_hip.h``).  ``regions``: the ``TextRegions`` (with ``gap``: the
    ``TextBlocks``) of the input, None inside ``TextEraser``.  ``rows``: numpy int32 ``[n, 16]``, ``(status, n, colour r, g, b, area, by0,
    bx0, by1, bx1, ay, ax, ry0, rx0, ry1, rx1)`` per row.  ``rect``: numpy int64 ``[n, 8]``, the inner rectangle in ``RegionGeometry.rect``'s
    layout (all 0 without one): ``region_crops`` and ``paste_crops`` take it as it is.  ``plane``: uint8 ``[H, W]`` of 0 / 255, the union of
    the balloons, or None.  ``table_rows``: the table where ``regions`` is None.  The properties are plain numpy on ``rows``."""
    regions: object
    rows: np.ndarray
    rect: np.ndarray
    plane: object = None
    table_rows: np.ndarray = None

    @property
    def table(self):
        """numpy int32 ``[n, 6]``: the region (block) table the rows belong to"""
        return self.table_rows if self.regions is None else self.regions.table

    @property
    def status(self):
        """int32 ``[n]``: bit 1 no ring, 2 the ring is not of one colour, 4 open, 8 the window is too large, 16 no pixels of its own"""
        return self.rows[:, 0]

    @property
    def is_balloon(self):
        """bool ``[n]``: the row has a balloon (open or closed): none of the bits 1, 2, 8 and 16"""
        return (self.rows[:, 0] & (1 | 2 | 8 | 16)) == 0

    @property
    def is_open(self):
        """bool ``[n]``: the fill ran to the end of its reach (lettering on open page)"""
        return (self.rows[:, 0] & 4) != 0

    @property
    def colour(self):
        """uint8 ``[n, 3]``: the rounded mean of the ring"""
        return self.rows[:, 2:5].astype(np.uint8)

    @property
    def ring_pixels(self):
        return self.rows[:, 1]

    @property
    def area(self):
        """int32 ``[n]``: the balloon's pixels, the row's own lettering included; 0 without a balloon"""
        return self.rows[:, 5]

    @property
    def box(self):
        """int32 ``[n, 4]``: ``y0, x0, y1, x1`` of the balloon, half-open"""
        return self.rows[:, 6:10]

    @property
    def anchor(self):
        """int32 ``[n, 2]``: ``(y, x)`` of the pixel of the lettering nearest the centre of its box"""
        return self.rows[:, 10:12]

    @property
    def inner(self):
        """int32 ``[n, 4]``: ``y0, x0, y1, x1``, half-open, of the largest upright rectangle inside the balloon that holds the anchor"""
        return self.rows[:, 12:16]

    def crops(self, page_u8, size, **kw):
        """``region_crops(page_u8, self.rect, size, **kw)``: the inner rectangles as slots to render into; the ``RegionCrops`` has ``crop(r)``
        and ``paste(page, slots)``"""
        return region_crops(page_u8, self.rect, size, **kw)


CROP_ORIENTS = {"upright": 0, "long": 1}
CROP_INFO = 10                                              # int32 words of info per slot
BALLOON_WORDS = 16                                          # int32 words per row of tsii_region_balloons


def _check_int_range(name, value, lo, hi):
    if isinstance(value, bool) or int(value) != value or not lo <= value <= hi:
        raise ValueError(f"{name} {value} must be an integer {lo}..{hi}")


def check_block_args(gap):
    _check_int_range("group gap", gap, 1, 64)


def check_region_args(connectivity, min_area, max_regions):
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity {connectivity} must be 4 or 8")
    if int(min_area) != min_area or min_area < 0:
        raise ValueError(f"min_area {min_area} must be an integer >= 0")
    if int(max_regions) != max_regions or max_regions < 1:
        raise ValueError(f"max_regions {max_regions} must be an integer >= 1")


def check_seed_args(min_seeds):
    _check_int_range("min_seeds", min_seeds, 1, 2 ** 31 - 1)


def check_flat_args(tol, ring):
    _check_int_range("flat tolerance", tol, 0, 255)
    _check_int_range("flat ring", ring, 1, 8)


def check_smooth_args(tol, ring, sweeps):
    _check_int_range("smooth tolerance", tol, 0, 255)
    _check_int_range("smooth ring", ring, 1, 8)
    try:
        check_sweeps(sweeps)
    except ValueError as e:
        raise ValueError(f"smooth {e}") from None


def check_tone_args(tol, ring, period):
    _check_int_range("tone tolerance", tol, 0, 255)
    _check_int_range("tone ring", ring, 1, 16)
    _check_int_range("tone period", period, 2, 16)


class RouteLayout:
    """The words of the ONE int32 tensor the flat, smooth and tone stages leave for the read-back, ``[core counts (nt) | found, kept |
    table (6 per row) | flat rows (5) | smooth rows (5) | tone rows (6)]`` with the rows of the enabled stages only: the only place that
    knows the offsets.  ``counts``, ``n_regions``, ``table`` and ``rows(name)`` are slices that work on the device tensor and on its host
    copy alike; ``tail``: the words behind the table, ``words``: all of them."""
    ROW_WORDS = {"flat": 5, "smooth": 5, "tone": 6}     # in the order the stages run

    def __init__(self, nt, max_regions, flat=False, smooth=False, tone=False):
        self.nt, self.max_regions = int(nt), int(max_regions)
        self.counts, self.n_regions = slice(0, self.nt), slice(self.nt, self.nt + 2)
        self.table = slice(self.nt + 2, self.nt + 2 + 6 * self.max_regions)
        self.stages = tuple(name for name, on in (("flat", flat), ("smooth", smooth), ("tone", tone)) if on)
        at, self._rows = self.table.stop, {}
        for name in self.stages:
            self._rows[name] = slice(at, at + self.ROW_WORDS[name] * self.max_regions)
            at = self._rows[name].stop
        self.tail, self.words = at - self.table.stop, at

    def rows(self, name):
        return self._rows[name]


class PageRead(NamedTuple):
    """What ``ReadBack.unpack`` finds in the host copy.  ``counts``: the core counts that select tiles (of the plane the last stage
    left).  ``table`` / ``found`` / ``kept`` / ``truncated``: the first labelling's (with ``group``: the blocks').  ``hull_area``,
    ``members`` / ``components``: with ``hull`` / ``group``, else None.  ``route_table`` (the components the flat, smooth and tone stages
    worked on), ``stages`` and ``gone`` as ``unpack_routes`` gives them: None, {} and None without such a stage.  ``plan_table`` /
    ``plan_truncated``: the regions that still hold text, for ``plan_fill_windows``.  ``seeds`` (the seed pixels of each table row),
    ``seed_dropped`` / ``seed_dropped_pixels`` (the rows ``tsii_region_seeds`` took out, their summed area): with ``seeds``, else None.
    ``n_vertices`` / ``vertices`` / ``rect``: with ``geometry``, of each table row (``RegionGeometry``), else None.
    ``crop_info``: with ``crops``, the ``info`` of the first ``min(rows, max_crops)`` table rows (``RegionCrops``), else None.
    ``balloon_rows``: with ``balloons``, int32 ``[rows, 16]`` of each table row (``RegionBalloons.rows``), else None.
    Without the regions path all but ``counts`` is None."""
    counts: np.ndarray
    table: np.ndarray = None
    found: int = None
    kept: int = None
    truncated: bool = None
    hull_area: np.ndarray = None
    members: np.ndarray = None
    components: int = None
    route_table: np.ndarray = None
    stages: dict = None
    gone: np.ndarray = None
    plan_table: np.ndarray = None
    plan_truncated: bool = None
    seeds: np.ndarray = None
    seed_dropped: int = None
    seed_dropped_pixels: int = None
    n_vertices: np.ndarray = None
    vertices: np.ndarray = None
    rect: np.ndarray = None
    crop_info: np.ndarray = None
    balloon_rows: np.ndarray = None


class ReadBack:
    """The ONE int32 tensor a page's only synchronisation copies, and the only place that knows its offsets: ``[first | second | members
    (max_regions), components]``.  ``first`` is the first labelling's tensor, ``[core counts (nt) | found, kept | table | tail]`` -- the
    blocks' with ``group`` -- whose ``tail`` words are the hull areas with ``hull``, else the route rows (``RouteLayout``).  ``second`` is
    there with ``hull`` and a route stage: the tensor of the labelling of the filled plane, in ``RouteLayout``'s form (``second_tail``
    words behind its table).  The last part is there with ``group``.  ``routes`` is the ``RouteLayout`` of the tensor the route stages
    work on, the second where there is one, else the first.  Without ``regions`` the tensor is the ``nt`` core counts alone.  With ``seeds``
    its LAST ``extra`` words are ``[seeds (max_regions) | dropped, dropped pixels]`` of ``tsii_region_seeds``: room the first labelling's
    tensor -- with ``group`` the blocks' ``whole`` -- is allocated with (``seed_room``), so that nothing in front of it moves.  With
    ``geometry`` (the ``max_vertices`` of the stage; 0: off) the tensor of ``_region_geometry`` (``GeometryLayout``) rides behind all of
    that, as the last ``geometry.words`` words.  With ``crops`` (the ``max_crops`` of the stage; 0: off) the ``info`` of ``_region_crops``
    rides behind that again: ``10 * max_crops`` words.  With ``balloons`` the rows of ``_region_balloons`` are the LAST ``16 * max_regions``
    words; without it the tensor has the length it had before that stage existed."""

    def __init__(self, nt, max_regions, hull=False, group=False, flat=False, smooth=False, tone=False, regions=True, seeds=False, geometry=0,
                 crops=0, balloons=False):
        n = int(max_regions)
        self.routes = RouteLayout(nt, n, flat, smooth, tone)
        self.regions, self.hull, self.group = bool(regions), bool(hull), bool(group)
        self.n_regions, self.second_tail = self.routes.n_regions, self.routes.tail
        self.tail = n if self.hull else self.routes.tail
        self.first = slice(0, self.routes.table.stop + self.tail)
        self.hull_area = slice(self.routes.table.stop, self.first.stop)
        two = self.hull and bool(self.routes.stages)
        self.own = slice(self.first.stop, self.first.stop + self.routes.words) if two else self.first
        self.members = slice(self.own.stop, self.own.stop + n)
        self.words = self.members.stop + 1 if self.group else self.own.stop if self.regions else int(nt)
        self.seeded = bool(seeds) and self.regions
        self.extra = n + 2 if self.seeded else 0
        self.seed_words, self.seed_dropped = slice(self.words, self.words + n), slice(self.words + n, self.words + self.extra)
        self.words += self.extra
        self.geometry = GeometryLayout(n, geometry) if geometry and self.regions else None
        self.geometry_words = slice(self.words, self.words + (self.geometry.words if self.geometry else 0))
        self.words = self.geometry_words.stop
        self.crops = int(crops) if crops and self.geometry is not None else 0
        self.crop_words = slice(self.words, self.words + CROP_INFO * self.crops)
        self.words = self.crop_words.stop
        self.balloons = bool(balloons) and self.regions
        self.balloon_words = slice(self.words, self.words + (BALLOON_WORDS * n if self.balloons else 0))
        self.words = self.balloon_words.stop

    def seed_room(self, whole):
        """(members, room) on the device for ``_region_seeds``: ``whole`` is the first labelling's tensor as allocated, ``[first | members,
        components (with group) | seeds, dropped]``; ``members`` is None without ``group``"""
        n = self.routes.max_regions
        assert self.seeded and whole.numel() == self.first.stop + (n + 1 if self.group else 0) + self.extra
        return (whole[self.first.stop:self.first.stop + n] if self.group else None), whole[whole.numel() - self.extra:]

    def join(self, first, second=None, whole=None, geometry=None, crops=None, balloons=None):
        """``_join`` of the stages' tensors, with the tensor of ``_region_geometry``, the ``info`` of ``_region_crops`` and the rows of
        ``_region_balloons`` behind it where those stages ran"""
        joined = self._join(first, second, whole)
        parts = [joined] + [t for t in (geometry, crops if geometry is not None else None, balloons) if t is not None]
        return joined if len(parts) == 1 else torch.cat(parts)

    def _join(self, first, second=None, whole=None):
        """the tensor to copy, from what the stages left on the device: ``first``, ``second`` (None where the route stages worked on
        ``first``) and, with ``group`` or ``seeds``, ``whole``: the tensor as allocated (``_text_blocks``', or ``_text_regions``' with the
        seeds' room behind it), whose front ``first`` is.  Copies only where a tensor has to
        ride between ``first`` and the members."""
        if second is None:
            return first if whole is None else whole
        return torch.cat([first, second] if whole is None else [first, second, whole[self.first.stop:]])

    def unpack(self, host) -> PageRead:
        """the host copy of the joined tensor -> ``PageRead``; ``host`` is not written, the tables and columns are copies"""
        if not self.regions:
            return PageRead(host, stages={})
        # with seeds: where the table was cut on entry, the count that is left reaches into empty rows (include/tsii_hip.h, K19)
        dropped = int(host[self.seed_dropped][0]) if self.seeded else 0
        counts, table, found, kept, truncated = unpack_regions(host[self.first], self.routes.nt, self.routes.max_regions, dropped)
        n = len(table)
        read = PageRead(counts, table, found, kept, truncated, stages={}, plan_table=table, plan_truncated=truncated)
        if self.hull:
            read = read._replace(hull_area=host[self.hull_area][:n].copy())
        if self.group:
            read = read._replace(members=host[self.members][:n].copy(), components=int(host[self.members.stop]))
        if self.routes.stages:                          # behind the hulls: the filled plane's own components; all that follows works on them
            counts, rtable, rtruncated, stages, gone = unpack_routes(host[self.own], self.routes, 0 if self.own != self.first else dropped)
            read = read._replace(counts=counts, route_table=rtable, stages=stages, gone=gone, plan_table=rtable[~gone], plan_truncated=rtruncated)
        if self.seeded:
            read = read._replace(seeds=host[self.seed_words][:n].copy(), seed_dropped=dropped,
                                 seed_dropped_pixels=int(host[self.seed_dropped][1]))
        if self.geometry is not None:
            read = read._replace(**dict(zip(("n_vertices", "vertices", "rect"), self.geometry.unpack(host[self.geometry_words], n))))
        if self.crops:
            read = read._replace(crop_info=host[self.crop_words].reshape(self.crops, CROP_INFO)[:min(n, self.crops)].copy())
        if self.balloons:
            read = read._replace(balloon_rows=host[self.balloon_words].reshape(self.routes.max_regions, BALLOON_WORDS)[:n].copy())
        return read


def _text_regions(text, connectivity, min_area, max_regions, grid=None, tail=0):
    """``tsii_text_regions`` in place on the device plane ``text`` -> (labels, packed): ``packed`` is ONE int32 device tensor
    ``[core counts (grid.count, with a grid) | found, kept | table rows | tail words]``, so that a caller reads everything back with
    one copy (``tail``: room behind the table for ``_region_hulls``)."""
    h, w = int(text.shape[0]), int(text.shape[1])
    _lib.check_device(text.new_empty(0, dtype=torch.float32))
    assert text.dtype == torch.uint8 and text.is_contiguous()
    nbytes = int(_lib.lib().tsii_text_regions_ws_bytes(h, w, int(max_regions)))
    if nbytes == 0:
        raise ValueError(f"text plane of {h} x {w} pixels is out of range")
    nt = 0 if grid is None else grid.count
    labels = torch.empty((h, w), dtype=torch.int32, device=text.device)
    packed = torch.zeros((nt + 2 + 6 * int(max_regions) + int(tail),), dtype=torch.int32, device=text.device)
    ws = ops._ws(nbytes, text)
    tile, halo = (0, 0) if grid is None else (grid.tile, grid.halo)
    call("tsii_text_regions", ptr(text), h, w, int(connectivity), int(min_area), int(max_regions), tile, halo,
         ptr(packed[:nt]) if nt else None, ptr(labels), ptr(packed[nt + 2:]), ptr(packed[nt:nt + 2]), ptr(ws), _lib.stream())
    return labels, packed


def _text_blocks(text, labels, counts, gap, min_area, max_regions, grid=None, tail=0, extra=0):
    """``tsii_text_blocks`` in place on the device plane ``text``, behind the ``_text_regions`` call (``min_area=0``, same ``grid``) that
    left ``labels`` and the device pair ``counts`` = its {found, kept} -> (block_labels, packed, whole).  ``packed`` has the layout
    ``_text_regions`` gives its own, ``[core counts | found, kept | table rows | tail words]``, of the BLOCKS: ``_region_hulls``
    and ``unpack_regions`` take it as it is, the flat, smooth and tone stages its slices (``RouteLayout``).  It is the front of ``whole``, the ONE tensor a caller reads back:
    ``[packed | members (max_regions) | the components found | extra words]`` (``extra``: room for ``_region_seeds``)."""
    h, w = int(text.shape[0]), int(text.shape[1])
    n = int(max_regions)
    assert text.dtype == torch.uint8 and text.is_contiguous() and labels.shape == text.shape and labels.dtype == torch.int32
    nbytes = int(_lib.lib().tsii_text_blocks_ws_bytes(h, w, n, int(gap)))
    if nbytes == 0:
        raise ValueError(f"text plane of {h} x {w} pixels, gap {gap}: out of range")
    nt = 0 if grid is None else grid.count
    front = nt + 2 + 6 * n + int(tail)
    block_labels = torch.empty((h, w), dtype=torch.int32, device=text.device)
    whole = torch.zeros((front + n + 1 + int(extra),), dtype=torch.int32, device=text.device)
    whole[front + n:front + n + 1].copy_(counts[:1])
    ws = ops._ws(nbytes, text)
    tile, halo = (0, 0) if grid is None else (grid.tile, grid.halo)
    call("tsii_text_blocks", ptr(text), ptr(labels), h, w, int(gap), int(min_area), n, tile, halo, ptr(whole[:nt]) if nt else None,
         ptr(block_labels), ptr(whole[nt + 2:]), ptr(whole[front:]), ptr(whole[nt:nt + 2]), ptr(ws), _lib.stream())
    return block_labels, whole[:front], whole


def _region_hulls(text, labels, packed, max_regions, grid=None):
    """``tsii_region_hulls`` in place on the device plane ``text``, right behind ``_text_regions`` (same ``grid``): ``packed`` is that
    call's tensor grown by a ``max_regions`` tail, ``[core counts | found, kept | table | hull_area]``; the core counts at its front
    are rewritten for the filled plane."""
    h, w = int(text.shape[0]), int(text.shape[1])
    nt = 0 if grid is None else grid.count
    n = int(max_regions)
    assert packed.numel() == nt + 2 + 7 * n and packed.dtype == torch.int32 and packed.device == text.device
    nbytes = int(_lib.lib().tsii_region_hulls_ws_bytes(h, w, n))
    if nbytes == 0:
        raise ValueError(f"text plane of {h} x {w} pixels is out of range")
    ws = ops._ws(nbytes, text)
    tile, halo = (0, 0) if grid is None else (grid.tile, grid.halo)
    call("tsii_region_hulls", ptr(text), ptr(labels), h, w, ptr(packed[nt + 2:]), ptr(packed[nt:nt + 2]), n, tile, halo,
         ptr(packed[:nt]) if nt else None, ptr(packed[nt + 2 + 6 * n:]), ptr(ws), _lib.stream())


class GeometryLayout:
    """The words of the ONE int32 tensor ``_region_geometry`` leaves for the read-back, ``[rect (16 per row: 8 int64) | n_vertices (1) |
    vertices (2 * max_vertices)]``: the rectangles stand first, so that they are 8-byte aligned in a tensor of their own."""

    def __init__(self, max_regions, max_vertices):
        n, m = int(max_regions), int(max_vertices)
        self.max_regions, self.max_vertices = n, m
        self.rect, self.n_vertices = slice(0, 16 * n), slice(16 * n, 17 * n)
        self.vertices = slice(17 * n, 17 * n + 2 * n * m)
        self.words = self.vertices.stop

    def unpack(self, host, rows):
        """host copy of the tensor -> (n_vertices ``[rows]``, vertices ``[rows, max_vertices, 2]``, rect int64 ``[rows, 8]``), copies; the
        vertex slots behind a row's count are 0, as the tensor was allocated"""
        rect = host[self.rect].copy().view(np.int64).reshape(self.max_regions, 8)[:rows].copy()
        vertices = host[self.vertices].reshape(self.max_regions, self.max_vertices, 2)[:rows].copy()
        return host[self.n_vertices][:rows].copy(), vertices, rect


def check_geometry_args(max_vertices):
    _check_int_range("max_vertices", max_vertices, 3, 1024)


def _region_geometry(labels, table, n_regions, max_regions, max_vertices):
    """``tsii_region_geometry`` on the current stream, behind ``_text_regions`` or ``_text_blocks``: ``labels``, ``table`` (the device words
    of the table) and ``n_regions`` (the device pair) as they left them, all read only -> the int32 device tensor of ``GeometryLayout``."""
    h, w = int(labels.shape[0]), int(labels.shape[1])
    lay = GeometryLayout(max_regions, max_vertices)
    assert labels.dtype == torch.int32 and labels.is_contiguous() and table.dtype == torch.int32 and table.numel() >= 6 * lay.max_regions
    nbytes = int(_lib.lib().tsii_region_geometry_ws_bytes(h, w, lay.max_regions, lay.max_vertices))
    if nbytes == 0:
        raise ValueError(f"region geometry: a page of {h} x {w} pixels (sides up to 32767), {max_regions} regions, {max_vertices} vertices: out of range")
    geo = torch.zeros((lay.words,), dtype=torch.int32, device=labels.device)
    ws = ops._ws(nbytes, labels)
    call("tsii_region_geometry", ptr(labels), ptr(table), ptr(n_regions), lay.max_regions, h, w, lay.max_vertices, ptr(geo[lay.n_vertices]),
         ptr(geo[lay.vertices]), ptr(geo[lay.rect]), ptr(ws), nbytes, _lib.stream())
    return geo


def check_crop_args(size, max_crops, orient, fill, supersample):
    try:
        ch, cw = size
    except (TypeError, ValueError):
        raise ValueError(f"crops {size!r} must be a pair (height, width) of the slots") from None
    _check_int_range("crops height", ch, 1, 4096)
    _check_int_range("crops width", cw, 1, 4096)
    _check_int_range("max_crops", max_crops, 1, 2 ** 31 - 1)
    if max_crops * ch * cw * 3 > 2 ** 31 - 1:
        raise ValueError(f"max_crops {max_crops} slots of {ch} x {cw} x 3 bytes: more than 2^31 - 1 bytes")
    if orient not in CROP_ORIENTS:
        raise ValueError(f"crop_orient {orient!r} must be one of {sorted(CROP_ORIENTS)}")
    _check_int_range("crop_fill", fill, 0, 255)
    _check_int_range("crop_supersample", supersample, 1, 4)


def _region_crops(page, rect, n_regions, max_regions, size, max_crops, orient, fill, supersample):
    """``tsii_region_crops`` on the current stream, behind ``_region_geometry``: ``page`` (uint8 ``[h, w, 3]``), ``rect`` (the device words
    of the rectangles, 8-byte aligned) and ``n_regions`` (the device pair) are read only -> (crops uint8 ``[max_crops, ch, cw, 3]``, info
    int32 ``[max_crops * 10]``) on the device; slots behind the rows served are ``fill``, their info 0."""
    h, w = int(page.shape[0]), int(page.shape[1])
    ch, cw = int(size[0]), int(size[1])
    assert page.dtype == torch.uint8 and page.is_contiguous() and page.dim() == 3 and page.shape[2] == 3
    assert rect.is_contiguous() and rect.numel() * rect.element_size() >= 64 * int(max_regions)
    crops = torch.full((int(max_crops), ch, cw, 3), int(fill), dtype=torch.uint8, device=page.device)
    info = torch.zeros((int(max_crops) * CROP_INFO,), dtype=torch.int32, device=page.device)
    call("tsii_region_crops", ptr(page), h, w, ptr(rect), ptr(n_regions), int(max_regions), int(max_crops), ch, cw, CROP_ORIENTS[orient], int(fill),
         int(supersample), ptr(info), ptr(crops), _lib.stream())
    return crops, info


def check_paste_args(slots_shape, info_shape, n_rows, supersample):
    """the shapes of ``paste_crops``: slots ``[n, ch, cw, 3 | 4]`` with sides 1..4096, info ``[n, 10]`` of the same ``n``, ``n_rows`` (None: all)
    in ``0..n`` -> the rows to serve"""
    slots_shape, info_shape = tuple(int(v) for v in slots_shape), tuple(int(v) for v in info_shape)
    if len(slots_shape) != 4 or slots_shape[3] not in (3, 4):
        raise ValueError(f"slots must be [n, ch, cw, 3 or 4] uint8, got {slots_shape}")
    if slots_shape[0] > 0:
        _check_int_range("slots height", slots_shape[1], 1, 4096)
        _check_int_range("slots width", slots_shape[2], 1, 4096)
    if len(info_shape) != 2 or info_shape[1] != CROP_INFO or info_shape[0] != slots_shape[0]:
        raise ValueError(f"info must be [n, {CROP_INFO}] int32 with a row per slot, got {info_shape} for slots of {slots_shape}")
    n = slots_shape[0] if n_rows is None else n_rows
    _check_int_range("n_rows", n, 0, slots_shape[0])
    _check_int_range("supersample", supersample, 1, 4)
    return int(n)


PASTE_PLAN = 12                                             # int64 words of plan per row


def _region_paste(page, info_d, n_d, slots, max_ss):
    """``tsii_region_paste`` on the current stream: ``page`` (uint8 ``[h, w, 3]``, on the device) is composited IN PLACE with ``slots`` (uint8
    ``[max_rows, ch, cw, 4]``, straight RGBA) along ``info_d`` (the device words of ``_region_crops``' info, ``10 * max_rows`` of them at
    least); ``n_d``: the device word of the row count -> plan int64 ``[max_rows, 12]`` on the device (row ``r``: live, the box ``y0, x0, y1,
    x1`` inclusive, the sub-samples per axis, the steps)."""
    h, w = int(page.shape[0]), int(page.shape[1])
    max_rows, ch, cw = int(slots.shape[0]), int(slots.shape[1]), int(slots.shape[2])
    assert page.dtype == torch.uint8 and page.is_contiguous() and page.dim() == 3 and page.shape[2] == 3
    assert slots.dtype == torch.uint8 and slots.is_contiguous() and slots.dim() == 4 and slots.shape[3] == 4 and slots.device == page.device
    assert info_d.dtype == torch.int32 and info_d.is_contiguous() and info_d.numel() >= CROP_INFO * max_rows and n_d.dtype == torch.int32
    plan = torch.zeros((max_rows, PASTE_PLAN), dtype=torch.int64, device=page.device)
    call("tsii_region_paste", ptr(page), h, w, ptr(info_d), ptr(n_d), max_rows, ptr(slots), ch, cw, int(max_ss), ptr(plan), _lib.stream())
    return plan


def _rgba(slots):
    """device slots ``[n, ch, cw, 3 | 4]`` -> contiguous RGBA: three channels are opaque"""
    if slots.shape[3] == 4:
        return slots.contiguous()
    return torch.cat([slots, torch.full_like(slots[..., :1], 255)], dim=3)


def balloon_rect_rows(rows):
    """balloon rows ``[n, 16]`` -> the ``rect`` rows ``tsii_region_balloons`` writes beside them, int64 ``[n, 8]``: they are a function of the
    inner rectangle, all 0 where there is none"""
    rows = np.asarray(rows).astype(np.int64).reshape(-1, BALLOON_WORDS)
    ry0, rx0, ry1, rx1 = rows[:, 12], rows[:, 13], rows[:, 14], rows[:, 15]
    rect = np.stack([np.full_like(ry0, -1), np.zeros_like(ry0), np.ones_like(ry0), rx0, rx1 - 1, -(ry1 - 1), -ry0, np.ones_like(ry0)], axis=1)
    rect[ry1 <= ry0] = 0
    return rect


def check_balloon_args(tol, ring, reach):
    _check_int_range("balloon tolerance", tol, 0, 255)
    _check_int_range("balloon ring", ring, 1, 8)
    _check_int_range("balloon reach", reach, ring, 512)


def _region_balloons(page, text, labels, table, n_regions, max_regions, ring, tol, reach, plane=False):
    """``tsii_region_balloons`` on the current stream, behind ``_text_regions`` or ``_text_blocks``: ``page`` (uint8 ``[h, w, 3]``), ``text``,
    ``labels``, ``table`` (the device words of the table) and ``n_regions`` (the device pair) are read only -> (rows int32 ``[16 *
    max_regions]``, rect int64 ``[max_regions, 8]``, plane uint8 ``[h, w]`` or None, sweeps int32 ``[max_regions]``: a view of the workspace's
    debug words, valid until the next call that takes a workspace) on the device; the rows behind those served are 0."""
    h, w = int(text.shape[0]), int(text.shape[1])
    n = int(max_regions)
    assert page.dtype == torch.uint8 and page.is_contiguous() and tuple(page.shape) == (h, w, 3) and page.device == text.device
    assert text.dtype == torch.uint8 and text.is_contiguous() and labels.shape == text.shape and labels.dtype == torch.int32 and labels.is_contiguous()
    assert table.dtype == torch.int32 and table.numel() >= 6 * n
    nbytes = int(_lib.lib().tsii_region_balloons_ws_bytes(h, w, n, int(reach)))
    if nbytes == 0:
        raise ValueError(f"region balloons: a page of {h} x {w} pixels (sides up to 32767), {max_regions} regions, reach {reach}: out of range")
    rows = torch.zeros((BALLOON_WORDS * n,), dtype=torch.int32, device=text.device)
    rect = torch.zeros((n, 8), dtype=torch.int64, device=text.device)
    out_plane = torch.empty((h, w), dtype=torch.uint8, device=text.device) if plane else None
    ws = ops._ws(nbytes, text)
    call("tsii_region_balloons", ptr(page), ptr(text), ptr(labels), h, w, ptr(table), ptr(n_regions), n, int(ring), int(tol), int(reach), ptr(rows),
         ptr(rect), ptr(out_plane), ptr(ws), _lib.stream())
    return rows, rect, out_plane, ws.view(torch.int32)[nbytes // 4 - n:nbytes // 4]


def _region_seeds(text, labels, seed, packed, room, max_regions, min_seeds, members=None, grid=None):
    """``tsii_region_seeds`` in place on the device planes ``text`` and ``labels``, right behind ``_text_regions`` or ``_text_blocks`` (same
    ``grid``): ``packed`` is that call's tensor, ``[core counts | found, kept | table | ...]``, whose table is compacted, whose kept count
    is lowered and whose core counts are rewritten for the reduced plane; ``members`` the blocks' column, compacted with the table;
    ``room``: ``max_regions + 2`` device words, ``[seeds | dropped, dropped pixels]``.  ``seed``: the uint8 seed plane, read only."""
    h, w = int(text.shape[0]), int(text.shape[1])
    nt = 0 if grid is None else grid.count
    n = int(max_regions)
    assert seed.shape == text.shape and all(t.dtype == torch.uint8 and t.is_contiguous() and t.device == text.device for t in (text, seed))
    assert labels.shape == text.shape and labels.dtype == torch.int32 and labels.is_contiguous()
    assert packed.numel() >= nt + 2 + 6 * n and room.numel() == n + 2 and all(t.dtype == torch.int32 and t.device == text.device for t in (packed, room))
    assert members is None or (members.numel() == n and members.dtype == torch.int32 and members.is_contiguous())
    nbytes = int(_lib.lib().tsii_region_seeds_ws_bytes(h, w, n))
    if nbytes == 0:
        raise ValueError(f"text plane of {h} x {w} pixels, {n} regions: out of range")
    ws = ops._ws(nbytes, text)
    tile, halo = (0, 0) if grid is None else (grid.tile, grid.halo)
    call("tsii_region_seeds", ptr(text), ptr(labels), ptr(seed), h, w, ptr(packed[nt + 2:]), ptr(packed[nt:nt + 2]), n, int(min_seeds), tile, halo,
         ptr(packed[:nt]) if nt else None, ptr(room[:n]), ptr(members), ptr(room[n:]), ptr(ws), _lib.stream())


def _flat_regions(page, text, labels, table, n_regions, rows, max_regions, ring, tol, painted, mask=None, grid=None, core_count=None):
    """``tsii_flat_regions`` on the current stream, in place on the device plane ``text``: ``labels``, ``table`` (the device words of the
    table) and ``n_regions`` (the device pair) as the ``_text_regions`` call that labelled THIS plane left them; ``rows``:
    ``5 * max_regions`` device words for the flat rows; ``core_count`` (with ``grid``) is rewritten for the reduced plane.  ``painted``
    (and ``mask``, the 0 / 255 plane of the text on entry) are written."""
    h, w = int(text.shape[0]), int(text.shape[1])
    n = int(max_regions)
    assert rows.numel() == 5 * n and rows.dtype == torch.int32 and rows.device == text.device and rows.is_contiguous()
    assert page.shape == (h, w, 3) and painted.shape == (h, w, 3) and all(t.dtype == torch.uint8 and t.is_contiguous() for t in (page, painted))
    assert mask is None or (mask.shape == (h, w) and mask.dtype == torch.uint8 and mask.is_contiguous())
    nbytes = int(_lib.lib().tsii_flat_regions_ws_bytes(h, w, n))
    if nbytes == 0:
        raise ValueError(f"text plane of {h} x {w} pixels is out of range")
    ws = ops._ws(nbytes, text)
    tile, halo = (0, 0) if grid is None else (grid.tile, grid.halo)
    call("tsii_flat_regions", ptr(page), ptr(text), ptr(labels), h, w, ptr(table), ptr(n_regions), n, int(ring), int(tol), tile, halo,
         ptr(core_count) if grid is not None else None, ptr(painted), ptr(mask), ptr(rows), ptr(ws), _lib.stream())


def _smooth_regions(page, text, labels, table, n_regions, rows, max_regions, ring, tol, sweeps, painted, mask=None, grid=None, core_count=None):
    """``tsii_smooth_regions_classify``, ``tsii_harmonic_fill`` on the whole page and ``tsii_smooth_regions_apply`` on the current stream,
    in place on the device plane ``text``: ``labels``, ``table`` (the device words of the table) and ``n_regions`` (the device pair) as the
    labelling -- or the flat stage behind it -- left them; ``rows``: ``5 * max_regions`` device words for the smooth rows; ``core_count``
    (with ``grid``) is rewritten for the reduced plane.  ``painted`` (and ``mask``, the 0 / 255 plane of the text on entry) are written."""
    h, w = int(text.shape[0]), int(text.shape[1])
    n = int(max_regions)
    assert rows.numel() == 5 * n and rows.dtype == torch.int32 and rows.device == text.device and rows.is_contiguous()
    assert page.shape == (h, w, 3) and painted.shape == (h, w, 3) and all(t.dtype == torch.uint8 and t.is_contiguous() for t in (page, painted, text))
    assert mask is None or (mask.shape == (h, w) and mask.dtype == torch.uint8 and mask.is_contiguous())
    nbytes = int(_lib.lib().tsii_smooth_regions_ws_bytes(h, w, n))
    if nbytes == 0:
        raise ValueError(f"text plane of {h} x {w} pixels is out of range")
    x = torch.empty((1, h, w, 3), dtype=torch.float32, device=text.device)
    valid = torch.empty((1, h, w), dtype=torch.float32, device=text.device)
    ws = ops._ws(nbytes, text)
    call("tsii_smooth_regions_classify", ptr(page), ptr(text), ptr(labels), h, w, ptr(table), ptr(n_regions), n, int(ring), int(tol), ptr(rows),
         ptr(x), ptr(valid), ptr(ws), _lib.stream())
    filled = _harmonic_fill(x, valid, int(sweeps))
    tile, halo = (0, 0) if grid is None else (grid.tile, grid.halo)
    call("tsii_smooth_regions_apply", ptr(page), ptr(text), ptr(labels), h, w, ptr(table), ptr(n_regions), n, ptr(rows), ptr(filled), tile, halo,
         ptr(core_count) if grid is not None else None, ptr(painted), ptr(mask), _lib.stream())


def _tone_regions(page, text, labels, table, n_regions, rows, max_regions, ring, period, tol, painted, mask=None, grid=None, core_count=None):
    """``tsii_tone_regions`` on the current stream, in place on the device plane ``text``: ``labels``, ``table`` (the device words of the
    table) and ``n_regions`` (the device pair) as the labelling -- or the flat and smooth stages behind it -- left them; ``rows``:
    ``6 * max_regions`` device words for the tone rows; ``core_count`` (with ``grid``) is rewritten for the reduced plane.  ``painted`` (and
    ``mask``, the 0 / 255 plane of the text on entry) are written."""
    h, w = int(text.shape[0]), int(text.shape[1])
    n = int(max_regions)
    assert rows.numel() == 6 * n and rows.dtype == torch.int32 and rows.device == text.device and rows.is_contiguous()
    assert page.shape == (h, w, 3) and painted.shape == (h, w, 3) and all(t.dtype == torch.uint8 and t.is_contiguous() for t in (page, painted, text))
    assert mask is None or (mask.shape == (h, w) and mask.dtype == torch.uint8 and mask.is_contiguous())
    nbytes = int(_lib.lib().tsii_tone_regions_ws_bytes(h, w, n, int(period)))
    if nbytes == 0:
        raise ValueError(f"text plane of {h} x {w} pixels, {n} regions, period {period}: out of range")
    ws = ops._ws(nbytes, text)
    tile, halo = (0, 0) if grid is None else (grid.tile, grid.halo)
    call("tsii_tone_regions", ptr(page), ptr(text), ptr(labels), h, w, ptr(table), ptr(n_regions), n, int(ring), int(period), int(tol), tile, halo,
         ptr(core_count) if grid is not None else None, ptr(painted), ptr(mask), ptr(rows), ptr(ws), _lib.stream())


def unpack_tone(rows_h, n):
    """host copy of the tone rows -> (is_tone bool ``[n]``, shift int32 ``[n, 2]``, err, step, ring_pixels int32 ``[n]``) of the ``n`` table
    rows in use"""
    rows = rows_h[:6 * n].reshape(n, 6)
    return rows[:, 0] != 0, rows[:, 1:3].copy(), rows[:, 3].copy(), rows[:, 5].copy(), rows[:, 4].copy()


def unpack_smooth(rows_h, n):
    """host copy of the smooth rows -> (is_smooth bool ``[n]``, step uint8 ``[n, 3]``, ring_pixels int32 ``[n]``) of the ``n`` table rows
    in use"""
    rows = rows_h[:5 * n].reshape(n, 5)
    return rows[:, 0] != 0, rows[:, 1:4].astype(np.uint8), rows[:, 4].copy()


def unpack_flat(rows_h, n):
    """host copy of the flat rows -> (is_flat bool ``[n]``, colour uint8 ``[n, 3]``, ring_pixels int32 ``[n]``) of the ``n`` table rows in
    use"""
    rows = rows_h[:5 * n].reshape(n, 5)
    return rows[:, 0] != 0, rows[:, 1:4].astype(np.uint8), rows[:, 4].copy()


def unpack_routes(own_h, layout, dropped=0):
    """host copy of the stages' tensor -> (core counts, table, truncated, stages, gone); ``dropped``: as for ``unpack_regions``.  ``stages``: per enabled stage the dict
    ``TextEraser.last_regions`` carries under its name (``table`` and the stage's columns: ``is_flat`` / ``colour`` / ``ring_pixels``, ...);
    ``gone``: bool per table row, some stage took the region out of the plane (it has no text left: its rows of the later stages are
    empty)."""
    counts_h, table, _, _, truncated = unpack_regions(own_h, layout.nt, layout.max_regions, dropped)
    columns = {"flat": (unpack_flat, ("is_flat", "colour", "ring_pixels")),
               "smooth": (unpack_smooth, ("is_smooth", "step", "ring_pixels")),
               "tone": (unpack_tone, ("is_tone", "shift", "err", "step", "ring_pixels"))}
    stages, gone = {}, np.zeros(len(table), bool)
    for name in layout.stages:
        unpack, names = columns[name]
        stages[name] = dict(zip(names, unpack(own_h[layout.rows(name)], len(table))), table=table)
        gone = gone | stages[name]["is_" + name]
    return counts_h, table, truncated, stages, gone


def unpack_regions(packed_h, nt, max_regions, dropped=0):
    """host copy of ``packed`` -> (core counts, table, found, kept, truncated).  ``dropped``: the rows ``tsii_region_seeds`` took out of the
    table behind the labelling: the table had ``min(kept + dropped, max_regions)`` rows then, and was cut if that is ``max_regions``."""
    found, kept = int(packed_h[nt]), int(packed_h[nt + 1])
    n = min(kept + int(dropped), int(max_regions)) - int(dropped)
    table = packed_h[nt + 2:nt + 2 + 6 * n].reshape(n, 6).copy()
    return packed_h[:nt], table, found, kept, kept > n


def _plane_on_device(text, device):
    t = torch.from_numpy(np.ascontiguousarray(text)) if isinstance(text, np.ndarray) else text
    if t.dim() != 2 or t.dtype != torch.uint8 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"text must be [H, W] uint8, got {tuple(t.shape)} {t.dtype}")
    dev = torch.device(device) if device is not None else (t.device if t.is_cuda else torch.device("cuda:0"))
    return t.to(dev, copy=True).contiguous()


def _like(result, text):
    """a device result as the same kind, on the same device, as the argument ``text``"""
    if isinstance(text, np.ndarray):
        return result.cpu().numpy()
    return result if result.device == text.device else result.to(text.device)


def fill_region_hulls(text, connectivity=8, min_area=0, max_regions=4096, device=None) -> RegionHulls:
    """The text plane with the convex hull of every kept region filled in: what the reference demo marks as "the text".  Arguments as
    for ``text_regions``; regions below ``min_area`` are dropped first (a hull may cover them again), kept regions beyond
    ``max_regions`` keep their own pixels and get no hull.  ``filled`` comes back the same kind and on the same device as ``text``,
    which is not modified; one synchronisation (the read-back of the counts, the table and the hull areas)."""
    check_region_args(connectivity, min_area, max_regions)
    plane = _plane_on_device(text, device)
    rb = ReadBack(0, max_regions, hull=True)
    labels, packed = _text_regions(plane, connectivity, min_area, max_regions, tail=rb.tail)
    _region_hulls(plane, labels, packed, max_regions)
    r = rb.unpack(packed.cpu().numpy())
    return RegionHulls(_like(plane * 255, text), TextRegions(_like(labels, text), r.table, r.found, r.kept, r.truncated), r.hull_area)


def _page_and_plane(page_u8, mask_u8, device):
    """the intake of the three fill functions: host or device arguments -> (page, plane) on one device, contiguous, the plane a copy"""
    p = torch.from_numpy(np.ascontiguousarray(page_u8)) if isinstance(page_u8, np.ndarray) else page_u8
    if p.dim() != 3 or p.dtype != torch.uint8 or tuple(p.shape) != tuple(mask_u8.shape[:2]) + (3,):
        raise ValueError(f"page must be [H, W, 3] uint8 for a mask of {tuple(mask_u8.shape)}, got {tuple(p.shape)} {p.dtype}")
    plane = _plane_on_device(mask_u8, device)
    return p.to(plane.device).contiguous(), plane


def flat_fill_regions(page_u8, mask_u8, tol, ring=3, connectivity=8, min_area=0, max_regions=4096, device=None) -> FlatFill:
    """Paint the text that sits on one flat colour.  ``page_u8``: ``[H, W, 3]`` uint8; ``mask_u8``: ``[H, W]`` uint8, non-zero = text (the
    255 masks ``TextEraser`` returns work directly); numpy or torch, host or device, neither is modified.  Regions below ``min_area`` are
    dropped first, as in ``text_regions``.  A kept region is FLAT when the page pixels within ``ring`` (1..8, Chebyshev distance) of it
    that are not text themselves differ by at most ``tol`` (0..255) grey levels in every channel; it is painted with their rounded mean
    colour and leaves ``rest``.  Regions without a ring, and kept regions beyond ``max_regions``, are never flat.  ``painted`` comes
    back the same kind and on the same device as ``page_u8``, ``rest`` and the labels as ``mask_u8``; one synchronisation (the read-back
    of the counts, the table and the flat rows).  Host arguments are computed on ``device`` (default ``cuda:0``)."""
    check_region_args(connectivity, min_area, max_regions)
    check_flat_args(tol, ring)
    page, plane = _page_and_plane(page_u8, mask_u8, device)
    lay = RouteLayout(0, max_regions, flat=True)
    labels, packed = _text_regions(plane, connectivity, min_area, lay.max_regions, tail=lay.tail)
    painted = torch.empty_like(page)
    _flat_regions(page, plane, labels, packed[lay.table], packed[lay.n_regions], packed[lay.rows("flat")], lay.max_regions, ring, tol, painted)
    packed_h = packed.cpu().numpy()
    _, table, found, kept, truncated = unpack_regions(packed_h, 0, lay.max_regions)
    is_flat, colour, ring_pixels = unpack_flat(packed_h[lay.rows("flat")], len(table))
    return FlatFill(_like(painted, page_u8), _like(plane * 255, mask_u8), TextRegions(_like(labels, mask_u8), table, found, kept, truncated),
                    is_flat, colour, ring_pixels)


def smooth_fill_regions(page_u8, mask_u8, tol, ring=3, sweeps=8, connectivity=8, min_area=0, max_regions=4096, device=None) -> SmoothFill:
    """Fill the text that sits on a smooth background.  ``page_u8``: ``[H, W, 3]`` uint8; ``mask_u8``: ``[H, W]`` uint8, non-zero = text (the
    255 masks ``TextEraser`` returns work directly); numpy or torch, host or device, neither is modified.  Regions below ``min_area`` are
    dropped first, as in ``text_regions``.  A kept region is SMOOTH when no page pixel within ``ring`` (1..8, Chebyshev distance) of it
    that is not text itself differs from a 4-neighbour that is not text by more than ``tol`` (0..255) grey levels in any channel: a
    gradient passes, a hard edge across the region does not.  It is filled with the harmonic continuation of the pixels around the
    text (``harmonic_fill`` on the whole page and the whole mask, ``sweeps`` 0..16: the same bytes) and leaves ``text``.  Regions without
    a ring, and kept regions beyond ``max_regions``, are never smooth.  ``painted`` comes back the same kind and on the same device as
    ``page_u8``, ``text`` as ``mask_u8``; one synchronisation (the read-back of the counts, the table and the smooth rows).  Host
    arguments are computed on ``device`` (default ``cuda:0``)."""
    check_region_args(connectivity, min_area, max_regions)
    check_smooth_args(tol, ring, sweeps)
    page, plane = _page_and_plane(page_u8, mask_u8, device)
    lay = RouteLayout(0, max_regions, smooth=True)
    labels, packed = _text_regions(plane, connectivity, min_area, lay.max_regions, tail=lay.tail)
    painted = torch.empty_like(page)
    _smooth_regions(page, plane, labels, packed[lay.table], packed[lay.n_regions], packed[lay.rows("smooth")], lay.max_regions, ring, tol, sweeps,
                    painted)
    packed_h = packed.cpu().numpy()
    _, table, _, _, _ = unpack_regions(packed_h, 0, lay.max_regions)
    is_smooth, step, ring_pixels = unpack_smooth(packed_h[lay.rows("smooth")], len(table))
    return SmoothFill(_like(painted, page_u8), _like(plane * 255, mask_u8), table, is_smooth, step, ring_pixels)


def tone_fill_regions(page_u8, mask_u8, tol, ring=8, period=12, connectivity=8, min_area=0, max_regions=4096, device=None) -> ToneFill:
    """Fill the text that sits on a periodic pattern.  ``page_u8``: ``[H, W, 3]`` uint8; ``mask_u8``: ``[H, W]`` uint8, non-zero = text (the
    255 masks ``TextEraser`` returns work directly); numpy or torch, host or device, neither is modified.  Regions below ``min_area`` are
    dropped first, as in ``text_regions``.  The ring of a kept region -- the page pixels within ``ring`` (1..16, Chebyshev distance) of it
    that are not text themselves -- is compared with the page under every shift of up to ``period`` (2..16) pixels along each axis.  The
    region is TONE when the ring is textured (two neighbouring pixels differ by more than ``tol`` somewhere), when under some shift of two
    pixels or more at least half the ring has a non-text partner and no such pair differs by more than ``tol`` (0..255) in any channel --
    the best such shift, then the shortest, is the region's period -- and when every text pixel of the region reaches a non-text pixel
    within 256 periods either way.  It is filled with those pixels and leaves ``text``.  The period must be a whole number of pixels;
    one outlier in the ring rejects a shift.  Regions without a ring, and kept regions beyond ``max_regions``, are never tone.
    ``painted`` comes back the same kind and on the same device as ``page_u8``, ``text`` as ``mask_u8``; one synchronisation (the
    read-back of the counts, the table and the tone rows).  Host arguments are computed on ``device`` (default ``cuda:0``)."""
    check_region_args(connectivity, min_area, max_regions)
    check_tone_args(tol, ring, period)
    page, plane = _page_and_plane(page_u8, mask_u8, device)
    lay = RouteLayout(0, max_regions, tone=True)
    labels, packed = _text_regions(plane, connectivity, min_area, lay.max_regions, tail=lay.tail)
    painted = torch.empty_like(page)
    _tone_regions(page, plane, labels, packed[lay.table], packed[lay.n_regions], packed[lay.rows("tone")], lay.max_regions, ring, period, tol,
                  painted)
    packed_h = packed.cpu().numpy()
    _, table, _, _, _ = unpack_regions(packed_h, 0, lay.max_regions)
    is_tone, shift, err, step, ring_pixels = unpack_tone(packed_h[lay.rows("tone")], len(table))
    return ToneFill(_like(painted, page_u8), _like(plane * 255, mask_u8), table, is_tone, shift, err, step, ring_pixels)


def text_blocks(mask_u8, gap, connectivity=8, min_area=0, max_regions=4096, device=None) -> TextBlocks:
    """Blocks of lettering in a text plane.  ``mask_u8``: ``[H, W]`` uint8, numpy or torch, host or device; non-zero = text (the 255 masks
    ``TextEraser`` returns work directly); it is not modified.  The connected regions (``connectivity`` 4 or 8) are grouped by single
    linkage: two regions are in one block when some pixel of one is within ``gap`` (1..64) pixels of some pixel of the other in both
    axes, directly or through other regions.  Blocks of fewer than ``min_area`` pixels are dropped -- a small mark beside a glyph stays,
    a speck on its own goes.  ``mask`` and ``labels`` come back the same kind and on the same device as ``mask_u8``; one
    synchronisation (the read-back of the counts, the table and the members).  A host plane is computed on ``device`` (default
    ``cuda:0``)."""
    check_region_args(connectivity, min_area, max_regions)
    check_block_args(gap)
    plane = _plane_on_device(mask_u8, device)
    labels, counts = _text_regions(plane, connectivity, 0, 0)
    block_labels, _, whole = _text_blocks(plane, labels, counts, gap, min_area, max_regions)
    r = ReadBack(0, max_regions, group=True).unpack(whole.cpu().numpy())
    return TextBlocks(_like(plane * 255, mask_u8), _like(block_labels, mask_u8), r.table, r.members, r.found, r.kept, r.components)


def seeded_regions(mask_u8, seed_u8, min_seeds=1, connectivity=8, min_area=0, gap=None, max_regions=4096, device=None) -> SeededRegions:
    """Hysteresis threshold on regions.  ``mask_u8``: ``[H, W]`` uint8, the plane cut at the LOW threshold; ``seed_u8``: the same shape, the
    plane cut at the HIGH one; numpy or torch, host or device, non-zero = set, neither is modified.  The connected regions of the mask
    (``connectivity`` 4 or 8) below ``min_area`` pixels are dropped first, as in ``text_regions``; a kept region then stays only if at least
    ``min_seeds`` of its pixels are seeds.  With ``min_seeds=1`` the mask that comes back is the classic hysteresis threshold: the
    components of the low plane that contain a high pixel.  With ``gap`` (1..64) the regions are grouped into blocks first, as in
    ``text_blocks``, and whole blocks are judged: a faint mark stays beside a confident glyph.  Kept regions beyond ``max_regions`` are not
    judged and stay.  ``mask`` and ``labels`` come back the same kind and on the same device as ``mask_u8``; one synchronisation (the
    read-back of the counts, the table and the seeds).  Host planes are computed on ``device`` (default ``cuda:0``)."""
    check_region_args(connectivity, min_area, max_regions)
    check_seed_args(min_seeds)
    if gap is not None:
        check_block_args(gap)
    plane = _plane_on_device(mask_u8, device)
    if tuple(seed_u8.shape) != tuple(plane.shape):
        raise ValueError(f"seed plane {tuple(seed_u8.shape)} for a mask of {tuple(plane.shape)}")
    seed = _plane_on_device(seed_u8, plane.device)
    rb = ReadBack(0, max_regions, group=gap is not None, seeds=True)
    if gap is None:
        labels, whole = _text_regions(plane, connectivity, min_area, max_regions, tail=rb.extra)
    else:
        every, counts = _text_regions(plane, connectivity, 0, 0)
        labels, _, whole = _text_blocks(plane, every, counts, gap, min_area, max_regions, extra=rb.extra)
    members, room = rb.seed_room(whole)
    _region_seeds(plane, labels, seed, whole[rb.first], room, max_regions, min_seeds, members)
    r = rb.unpack(whole.cpu().numpy())
    return SeededRegions(_like(plane * 255, mask_u8), _like(labels, mask_u8), r.table, r.seeds, r.found, r.kept, r.seed_dropped,
                         r.seed_dropped_pixels, r.truncated, r.members)


def region_geometry(mask_u8, connectivity=8, min_area=0, max_regions=4096, max_vertices=64, gap=None, device=None) -> RegionGeometry:
    """The hull polygon and the minimum-area enclosing rectangle of every text region: ``cv2.convexHull`` and ``cv2.minAreaRect`` per region,
    on the device and in integers.  ``mask_u8``: ``[H, W]`` uint8, numpy or torch, host or device, sides up to 32767; non-zero = text (the 255
    masks ``TextEraser`` returns work directly); it is not modified.  Regions below ``min_area`` are dropped first, as in ``text_regions``;
    with ``gap`` (1..64) the regions are grouped into blocks first, as in ``text_blocks``, and ``regions`` is the ``TextBlocks``.  Up to
    ``max_vertices`` (3..1024) vertices per row come back; ``n_vertices`` is the true count and the rectangle is always that of the whole
    hull.  Kept regions beyond ``max_regions`` get no geometry.  Labels come back the same kind and on the same device as ``mask_u8``; one
    synchronisation (the read-back of the counts, the table, the vertices and the rectangles).  A host plane is computed on ``device``
    (default ``cuda:0``)."""
    check_region_args(connectivity, min_area, max_regions)
    check_geometry_args(max_vertices)
    if gap is not None:
        check_block_args(gap)
    plane = _plane_on_device(mask_u8, device)
    rb = ReadBack(0, max_regions, group=gap is not None, geometry=max_vertices)
    if gap is None:
        labels, first = _text_regions(plane, connectivity, min_area, max_regions)
        whole = None
    else:
        every, counts = _text_regions(plane, connectivity, 0, 0)
        labels, first, whole = _text_blocks(plane, every, counts, gap, min_area, max_regions)
    geo = _region_geometry(labels, first[rb.routes.table], first[rb.n_regions], max_regions, max_vertices)
    r = rb.unpack(rb.join(first, None, whole, geo).cpu().numpy())
    if gap is None:
        regions = TextRegions(_like(labels, mask_u8), r.table, r.found, r.kept, r.truncated)
    else:
        regions = TextBlocks(_like(plane * 255, mask_u8), _like(labels, mask_u8), r.table, r.members, r.found, r.kept, r.components)
    return RegionGeometry(regions, r.n_vertices, r.vertices, r.rect)


def region_balloons(page_u8, mask_u8, tol, ring=3, reach=256, connectivity=8, min_area=0, gap=None, return_plane=False, max_regions=4096,
                    device=None) -> RegionBalloons:
    """The speech balloon around every text region, and the room for a translation inside it.  ``page_u8``: ``[H, W, 3]`` uint8; ``mask_u8``:
    ``[H, W]`` uint8, non-zero = text (the 255 masks ``TextEraser`` returns work directly); numpy or torch, host or device, sides up to
    32767, neither is modified.  Regions below ``min_area`` are dropped first, as in ``text_regions``; with ``gap`` (1..64) the regions are
    grouped into blocks first, as in ``text_blocks``, and ``regions`` is the ``TextBlocks``.  Per row: the ring within ``ring`` (1..8) pixels
    of the lettering gives the colour, as in ``flat_fill_regions``; where it is of one colour within ``tol`` (0..255) the balloon is the
    flood fill (4-connected) from the lettering over the pixels within ``tol`` of that colour that are no text, inside the row's box grown
    by ``reach`` (``ring``..512) pixels; other rows' lettering is an obstacle.  ``is_open`` says that the fill ran to the end of its reach
    (lettering on open page), ``inner`` is the largest upright rectangle in the balloon around the block's centre and ``rect`` the same in
    the layout ``region_crops`` takes.  A row whose window would exceed 1024 pixels a side gets status bit 8 and no balloon.
    ``plane`` (with ``return_plane``) and the labels come back the same kind and on the same device as ``mask_u8``; one synchronisation
    (the read-back of the counts, the table and the balloon rows).  Host arguments are computed on ``device`` (default ``cuda:0``)."""
    check_region_args(connectivity, min_area, max_regions)
    check_balloon_args(tol, ring, reach)
    if gap is not None:
        check_block_args(gap)
    page, plane = _page_and_plane(page_u8, mask_u8, device)
    rb = ReadBack(0, max_regions, group=gap is not None, balloons=True)
    if gap is None:
        labels, first = _text_regions(plane, connectivity, min_area, max_regions)
        whole = None
    else:
        every, counts = _text_regions(plane, connectivity, 0, 0)
        labels, first, whole = _text_blocks(plane, every, counts, gap, min_area, max_regions)
    rows, _, filled, _ = _region_balloons(page, plane, labels, first[rb.routes.table], first[rb.n_regions], max_regions, ring, tol, reach,
                                             plane=return_plane)
    r = rb.unpack(rb.join(first, None, whole, balloons=rows).cpu().numpy())
    if gap is None:
        regions = TextRegions(_like(labels, mask_u8), r.table, r.found, r.kept, r.truncated)
    else:
        regions = TextBlocks(_like(plane * 255, mask_u8), _like(labels, mask_u8), r.table, r.members, r.found, r.kept, r.components)
    return RegionBalloons(regions, r.balloon_rows, balloon_rect_rows(r.balloon_rows), None if filled is None else _like(filled, mask_u8))


def region_crops(page_u8, rect, size, n_rows=None, orient="upright", fill=255, supersample=4, device=None) -> RegionCrops:
    """Rectified crops of a page's text regions: every row of ``rect`` -- the ``rect`` of a ``RegionGeometry``, int64 ``[n, 8]``, numpy or
    torch -- is cut out of ``page_u8`` (``[H, W, 3]`` uint8, numpy or torch, host or device, sides up to 32767; not modified) along its
    padded minimum-area rectangle, deskewed and scaled to fit a slot of ``size = (ch, cw)`` pixels (sides 1..4096) with its aspect ratio
    kept: bilinear, up to ``supersample`` (1..4) squared sub-samples per pixel where the block is reduced, all in integers.
    ``orient="upright"`` turns a block by at most 45 degrees, so a column stays tall; ``"long"`` lays the longer side along the slot's
    width, so a column reads rightwards.  The first ``n_rows`` rows (default: all) are served.  ``crops`` comes back the same kind and on
    the same device as the page, ``n_rows * ch * cw * 3`` bytes; one synchronisation (the read-back of ``info``).  A host page is worked
    on on ``device`` (default ``cuda:0``)."""
    rows = np.asarray(rect.cpu() if isinstance(rect, torch.Tensor) else rect)
    if rows.ndim != 2 or rows.shape[1] != 8 or rows.dtype != np.int64:
        raise ValueError(f"rect must be [n, 8] int64, got {rows.shape} {rows.dtype}")
    n = len(rows) if n_rows is None else n_rows
    _check_int_range("n_rows", n, 0, len(rows))
    check_crop_args(size, max(n, 1), orient, fill, supersample)
    p = torch.from_numpy(np.ascontiguousarray(page_u8)) if isinstance(page_u8, np.ndarray) else page_u8
    if p.dim() != 3 or p.dtype != torch.uint8 or p.shape[2] != 3 or not 1 <= p.shape[0] <= 32767 or not 1 <= p.shape[1] <= 32767:
        raise ValueError(f"page must be [H, W, 3] uint8 with sides 1..32767, got {tuple(p.shape)} {p.dtype}")
    dev = torch.device(device) if device is not None else (p.device if p.is_cuda else torch.device("cuda:0"))
    if n == 0:
        return RegionCrops(_like(torch.zeros((0, int(size[0]), int(size[1]), 3), dtype=torch.uint8, device=dev), page_u8), np.zeros((0, CROP_INFO), np.int32))
    rect_d = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
    count = torch.tensor([n, n], dtype=torch.int32, device=dev)
    crops, info = _region_crops(p.to(dev).contiguous(), rect_d, count, len(rows), size, n, orient, fill, supersample)
    return RegionCrops(_like(crops, page_u8), info.cpu().numpy().reshape(n, CROP_INFO))


def paste_crops(page_u8, slots, info, n_rows=None, supersample=4, device=None):
    """Pictures laid back onto a page where ``region_crops`` cut them out: the return trip a typesetter needs.  ``page_u8``: ``[H, W, 3]``
    uint8, numpy or torch, host or device, sides up to 32767; it is not modified, the result is a copy of the same kind and on the same
    device.  ``slots``: ``[n, ch, cw, 4]`` uint8, straight (not premultiplied) RGBA, or ``[n, ch, cw, 3]``, which is opaque; the picture of row
    ``r`` is its top-left ``uh x uw`` pixels, the rest of the slot is ignored.  ``info``: ``[n, 10]`` int32, numpy or torch: ``RegionCrops.info``
    (or the device tensor behind it), which says where each slot came from.  The first ``n_rows`` rows (default: all) are pasted in
    ascending order, a later one over an earlier one; rows without pixels paste nothing.  Bilinear in integers, with up to ``supersample``
    (1..4) squared sub-samples per page pixel where the picture is reduced; the picture's rim is antialiased against the page.  No
    synchronisation beyond the copies of a host page.  A host page is worked on on ``device`` (default ``cuda:0``)."""
    p = torch.from_numpy(np.ascontiguousarray(page_u8)) if isinstance(page_u8, np.ndarray) else page_u8
    if p.dim() != 3 or p.dtype != torch.uint8 or p.shape[2] != 3 or not 1 <= p.shape[0] <= 32767 or not 1 <= p.shape[1] <= 32767:
        raise ValueError(f"page must be [H, W, 3] uint8 with sides 1..32767, got {tuple(p.shape)} {p.dtype}")
    sl = torch.from_numpy(np.ascontiguousarray(slots)) if isinstance(slots, np.ndarray) else slots
    rows = torch.from_numpy(np.ascontiguousarray(info)) if isinstance(info, np.ndarray) else info
    if sl.dtype != torch.uint8 or rows.dtype != torch.int32:
        raise ValueError(f"slots must be uint8 and info int32, got {sl.dtype} and {rows.dtype}")
    n = check_paste_args(sl.shape, rows.shape, n_rows, supersample)
    dev = torch.device(device) if device is not None else (p.device if p.is_cuda else torch.device("cuda:0"))
    out = p.to(dev, copy=True).contiguous()
    if n > 0:
        count = torch.tensor([n], dtype=torch.int32, device=dev)
        _region_paste(out, rows.to(dev).contiguous().reshape(-1), count, _rgba(sl.to(dev)), supersample)
    return _like(out, page_u8)


def text_regions(text, connectivity=8, min_area=0, max_regions=4096, device=None) -> TextRegions:
    """Connected regions of a text plane.  ``text``: ``[H, W]`` uint8, numpy or torch, host or device; non-zero = text (the 255
    masks ``TextEraser`` returns work directly).  The argument is not modified.  Regions of fewer than ``min_area`` pixels are
    dropped.  ``labels`` comes back the same kind and on the same device as ``text``; one synchronisation (the read-back of the
    counts and the table).  A host plane is computed on ``device`` (default ``cuda:0``)."""
    check_region_args(connectivity, min_area, max_regions)
    plane = _plane_on_device(text, device)
    labels, packed = _text_regions(plane, connectivity, min_area, max_regions)
    _, table, found, kept, truncated = unpack_regions(packed.cpu().numpy(), 0, max_regions)
    return TextRegions(_like(labels, text), table, found, kept, truncated)

