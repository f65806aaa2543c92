"""Page-level text removal: segment -> mask -> inpaint -> compose (the reference README's road, run end to end).

``TextEraser`` cuts a uint8 page of any size into overlapping square tiles, runs a segmentation net on them, turns the logits
into a dilated text plane, sends only the tiles that contain text through an inpainting net, and writes the inpainted pixels back
into the page bytes.  The page is uploaded once as uint8 and downloaded once as uint8; everything between stays on the device, in
the kernels of ``csrc/pipeline.hip`` (semantics: ``include/tsii_hip.h``, "K8: page pipeline") and the two nets.  Inference
only: nothing here records autograd.

With ``seg_long_side`` the segmenter works at its own resolution, as the reference's ``EvaluateSet`` has it: the page is resized on
the device with Pillow's bicubic filter, byte for byte, and the working-resolution text plane comes back onto the page's grid with
"bilinear, then ``> 0``" in integers (``csrc/resample.hip``; "K11: working resolution").  The inpainting net always sees the page's
own pixels.

With ``pack`` the filler's tiles are no longer those of the grid that have text but windows centred on the text regions, placed on the
host by ``plan_fill_windows`` from the region boxes that the page's one synchronisation brings back anyway.

With ``flat`` the text regions that sit on one flat colour -- lettering in a speech bubble -- are painted with that colour on the device
(``csrc/flat.hip``; "K13: flat regions") and never reach the filler: the reference README's "use the generated mask to white out
words", applied where nothing has to be inferred.

With ``smooth`` the regions whose surroundings are locally smooth -- lettering on a gradient, a soft shadow, a sky -- are filled with the
harmonic continuation of those surroundings at page level (``csrc/smooth.hip``; "K16: smooth regions", around the solver of
``csrc/harmonic.hip``) and never reach the filler either: flat, then smooth, then the net, decided per region on the device.

With ``tone`` the regions whose surroundings are a periodic pattern -- lettering on screentone, stripes, a dot lattice -- are filled by copying
the pixel a whole number of periods away (``csrc/tone.hip``; "K17: tone regions"): flat, then smooth, then tone, then the net.

With ``group`` the regions are first grouped into blocks of lettering on the device (``csrc/blocks.hip``; "K15: text blocks"): the area
filter, the hulls, the flat stage and ``pack`` then judge, fill, paint and place whole blocks instead of single glyphs.

With ``seed`` the one cut at ``threshold`` becomes a hysteresis threshold: a region (with ``group``: a block) stays text only if the
segmenter was sure, at the probability ``seed``, somewhere inside it (``csrc/seeds.hip``; "K19: seeded regions").  What is dropped leaves the
plane, the labels and the table on the device, in front of the hulls, the routes and the page's one synchronisation.

With ``blend`` the pixels the filler paints are taken into the page in the gradient domain (``csrc/blend.hip``; "K20: seamless fill", around
the solver of ``csrc/harmonic.hip``): the filler's error at the valid pixels of each tile, continued harmonically into the holes, is added
there between the filler and compose.
"""
from contextlib import contextmanager
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np
import torch
from torch import nn

from . import _lib
from ._lib import call, ptr
from .BaseModels import to_nhwc
from .fill import _seamless_fill, check_sweeps
from .masks import MaskParts
from .regions import (ReadBack, RegionBalloons, RegionCrops, _check_int_range, _flat_regions, _region_balloons, _region_crops, _region_geometry,
                      _region_hulls, _region_paste, _region_seeds, _rgba, _smooth_regions, _text_blocks, _text_regions, _tone_regions,
                      balloon_rect_rows, check_balloon_args, check_block_args, check_crop_args, check_flat_args, check_geometry_args,
                      check_region_args, check_seed_args, check_smooth_args, check_tone_args)


class TileGrid(NamedTuple):
    """Tiling of an ``h x w`` page: ``ty * tx`` tiles of ``tile`` pixels a side in row-major order; tile ``(i, j)`` starts at page
    row ``i * stride - halo`` / column ``j * stride - halo`` and owns the core ``[i * stride, (i + 1) * stride)`` x
    ``[j * stride, (j + 1) * stride)`` clipped to the page."""
    h: int
    w: int
    tile: int
    halo: int
    stride: int
    ty: int
    tx: int

    @property
    def count(self):
        return self.ty * self.tx

    def origin(self, t):
        """Page (row, column) of the first pixel of tile ``t`` (negative on the first row / column of tiles when halo > 0)."""
        return (t // self.tx) * self.stride - self.halo, (t % self.tx) * self.stride - self.halo

    def core(self, t):
        """(y0, y1, x0, x1): the page pixels tile ``t`` owns."""
        i, j = t // self.tx, t % self.tx
        return (i * self.stride, min((i + 1) * self.stride, self.h), j * self.stride, min((j + 1) * self.stride, self.w))


def tile_grid(h, w, tile, halo) -> TileGrid:
    h, w, tile, halo = int(h), int(w), int(tile), int(halo)
    if h < 1 or w < 1:
        raise ValueError(f"page of {h} x {w} pixels")
    if tile < 32 or tile % 32 or halo < 0 or tile - 2 * halo <= 0:
        raise ValueError(f"tile {tile} must be a multiple of 32 and larger than 2 * halo ({halo})")
    s = tile - 2 * halo
    return TileGrid(h, w, tile, halo, s, -(-h // s), -(-w // s))


# ---- thin wrappers of the tsii_* entry points (no autograd; byte planes are uint8, counts / tile lists int32) ----------------------
def _same_device(*ts):
    # no CPU path: host tensors are refused here (the empty fp32 tensor carries the device of the byte / int planes into the check)
    _lib.check_device(ts[0].new_empty(0, dtype=torch.float32), *[t for t in ts if t.is_floating_point()])
    assert all(t.device == ts[0].device and t.is_contiguous() for t in ts)


def _page_tiles_norm(page, g: TileGrid, scale, shift):
    tiles = torch.empty((g.count, g.tile, g.tile, 3), dtype=torch.float32, device=page.device)
    _same_device(page, tiles)
    call("tsii_page_tiles_norm", ptr(page), g.h, g.w, g.tile, g.halo, *[float(v) for v in scale], *[float(v) for v in shift],
         ptr(tiles), _lib.stream())
    return tiles


def _tiles_text_mask(logits, g: TileGrid, logit_threshold, dilate):
    assert logits.shape == (g.count, g.tile, g.tile)
    text = torch.empty((g.h, g.w), dtype=torch.uint8, device=logits.device)
    counts = torch.empty((g.count,), dtype=torch.int32, device=logits.device)
    _same_device(logits, text, counts)
    call("tsii_tiles_text_mask", ptr(logits), g.h, g.w, g.tile, g.halo, float(logit_threshold), int(dilate), ptr(text), ptr(counts),
         _lib.stream())
    return text, counts


def _page_tiles_fill(page, text, g: TileGrid, tile_ids):
    ns = int(tile_ids.numel())
    img = torch.empty((ns, g.tile, g.tile, 3), dtype=torch.float32, device=page.device)
    mask = torch.empty((ns, g.tile, g.tile), dtype=torch.float32, device=page.device)
    _same_device(img, mask, page, text, tile_ids)
    call("tsii_page_tiles_fill", ptr(page), ptr(text), g.h, g.w, g.tile, g.halo, ptr(tile_ids), ns, ptr(img), ptr(mask), _lib.stream())
    return img, mask


def _compose_page_u8(page, text, out, slot, g: TileGrid, clean, mask_u8):
    ns = 0 if out is None else int(out.shape[0])
    assert out is None or out.shape == (ns, g.tile, g.tile, 3)
    _same_device(page, text, clean, mask_u8, *([] if out is None else [out, slot]))
    call("tsii_compose_page_u8", ptr(page), ptr(text), ptr(out), ptr(slot), ns, g.h, g.w, g.tile, g.halo, ptr(clean), ptr(mask_u8),
         _lib.stream())


def _page_windows_fill(page, text, g: TileGrid, origin):
    n = int(origin.shape[0])
    img = torch.empty((n, g.tile, g.tile, 3), dtype=torch.float32, device=page.device)
    mask = torch.empty((n, g.tile, g.tile), dtype=torch.float32, device=page.device)
    _same_device(img, mask, page, text, origin)
    call("tsii_page_windows_fill", ptr(page), ptr(text), g.h, g.w, g.tile, ptr(origin), n, ptr(img), ptr(mask), _lib.stream())
    return img, mask


def _compose_page_windows_u8(page, text, out, origin, rect, g: TileGrid, clean, mask_u8):
    n = int(out.shape[0])
    assert out.shape == (n, g.tile, g.tile, 3) and origin.shape == (n, 2) and rect.shape == (n, 4)
    _same_device(page, text, clean, mask_u8, out, origin, rect)
    call("tsii_compose_page_windows_u8", ptr(page), ptr(text), ptr(out), ptr(origin), ptr(rect), n, g.h, g.w, g.tile, ptr(clean),
         ptr(mask_u8), _lib.stream())


MAX_FILL_WINDOWS = 1024         # what tsii_compose_page_windows_u8 accepts


def plan_fill_windows(boxes, h, w, tile, halo):
    """Filler windows for the text regions of an ``h x w`` page: ``(origins, rects)``, int32 ``[m, 2]`` (page row and column of each
    window's first pixel) and int32 ``[m, 4]`` (``y0, x0, y1, x1``, half-open: the page rectangle each window owns).  ``boxes``: int
    ``[n, 4]`` of ``(y0, x0, y1, x1)``, half-open, inside the page -- the box columns of a region table.  Pure host code.

    With ``S = tile - 2 * halo``: the rects cover every box; each is non-empty, inside the page, at most ``S`` a side and inside its
    window, at least ``halo`` pixels from every window edge that is not at or beyond the page edge.  Where the page side is at least
    ``tile`` the origin lies in ``[0, side - tile]`` (no window pixel is spent beyond the page), else it is ``-((tile - side) // 2)``.
    Rects of different windows may overlap; the lowest index owns a pixel.  The same boxes give the same windows.

    Greedy: boxes larger than ``S`` are cut into ``S x S`` pieces from their own corner; the pieces, sorted by ``(y0, x0)``, each join
    the first window whose bounding box stays within ``S x S`` with them, or open a new one; a window is centred on its box."""
    g = tile_grid(h, w, tile, halo)
    s = g.stride
    boxes = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    pieces = []
    for y0, x0, y1, x1 in boxes.tolist():
        if not (0 <= y0 < y1 <= g.h and 0 <= x0 < x1 <= g.w):
            raise ValueError(f"box ({y0}, {x0}, {y1}, {x1}) is empty or leaves the {g.h} x {g.w} page")
        pieces += [(py, px, min(py + s, y1), min(px + s, x1)) for py in range(y0, y1, s) for px in range(x0, x1, s)]
    pieces.sort()
    wins, first_open = [], 0        # windows before first_open start S rows or more above the current piece: nothing can join them any more
    for y0, x0, y1, x1 in pieces:
        while first_open < len(wins) and wins[first_open][0] + s <= y0:
            first_open += 1
        for win in wins[first_open:]:
            u = (win[0], min(win[1], x0), max(win[2], y1), max(win[3], x1))      # win[0] <= y0: the pieces come sorted
            if u[2] - u[0] <= s and u[3] - u[1] <= s:
                win[:] = u
                break
        else:
            wins.append([y0, x0, y1, x1])
    rects = np.asarray(wins, dtype=np.int32).reshape(-1, 4)

    def origin(start, extent, side):
        if side < tile:
            return np.full_like(start, -((tile - side) // 2))
        return np.clip(start - (tile - extent) // 2, 0, side - tile)
    origins = np.stack([origin(rects[:, 0], rects[:, 2] - rects[:, 0], g.h), origin(rects[:, 1], rects[:, 3] - rects[:, 1], g.w)], axis=1)
    return origins.astype(np.int32), rects


def working_size(h, w, long_side):
    """``(hs, ws)``: the size ``EvaluateSet(resize=long_side)`` resizes an ``h x w`` page to before it pads (Dataloader.py:285-317):
    ``int(side * (long_side / max(h, w))) // 8 * 8`` per side -- and at least 8, where the reference would ask Pillow for an empty image."""
    ratio = int(long_side) / max(int(h), int(w))
    return tuple(max(8, int(x * ratio) // 8 * 8) for x in (int(h), int(w)))


RESIZE_MAX_RATIO = 8            # per axis, either way: what tsii_page_resize_u8 accepts (a table row of at most 33 taps)
_RESIZE_TABLES = {}             # (in, out, device) -> (bounds [out, 2], kk [out, taps], taps) on the device


def _check_resize(h, w, hs, ws):
    for a, b in ((h, hs), (w, ws)):
        if a < 1 or b < 1 or a > RESIZE_MAX_RATIO * b or b > RESIZE_MAX_RATIO * a:
            raise ValueError(f"resize {h} x {w} -> {hs} x {ws}: every side >= 1 and within {RESIZE_MAX_RATIO} x of its counterpart")


def _resize_tables(n_in, n_out, device):
    """device copies of ``tsii_resize_coeffs_u8``'s tables for one axis, made once per (in, out) pair and device"""
    key = (int(n_in), int(n_out), str(device))
    hit = _RESIZE_TABLES.get(key)
    if hit is None:
        taps = int(_lib.lib().tsii_resize_taps(key[0], key[1]))
        if taps == 0:
            raise ValueError(f"resize {n_in} -> {n_out} is out of range")
        bounds, kk = np.zeros((key[1], 2), np.int32), np.zeros((key[1], taps), np.int32)
        call("tsii_resize_coeffs_u8", key[0], key[1], bounds.ctypes.data, kk.ctypes.data)      # a host function: host arrays
        hit = _RESIZE_TABLES[key] = (torch.from_numpy(bounds).to(device), torch.from_numpy(kk).to(device), taps)
    return hit


def _page_resize_u8(page, hs, ws):
    """device page ``[H, W, 3]`` uint8 -> ``[hs, ws, 3]`` uint8 (``tsii_page_resize_u8``)"""
    h, w = int(page.shape[0]), int(page.shape[1])
    _check_resize(h, w, hs, ws)
    by, ky, ty = _resize_tables(h, hs, page.device) if h != hs else (None, None, 0)
    bx, kx, tx = _resize_tables(w, ws, page.device) if w != ws else (None, None, 0)
    out = torch.empty((hs, ws, 3), dtype=torch.uint8, device=page.device)
    _same_device(page, out, *[t for t in (by, ky, bx, kx) if t is not None])
    call("tsii_page_resize_u8", ptr(page), h, w, int(hs), int(ws), ptr(by), ptr(ky), ptr(bx), ptr(kx), ty, tx, ptr(out), _lib.stream())
    return out


def _page_tensor(page_u8):
    """a page as the caller gives it, numpy or torch -> the torch tensor of it, checked: ``[H, W, 3]`` uint8 with ``H, W >= 1``"""
    t = torch.from_numpy(np.ascontiguousarray(page_u8)) if isinstance(page_u8, np.ndarray) else page_u8
    if t.dim() != 3 or t.shape[2] != 3 or t.dtype != torch.uint8 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"page must be [H, W, 3] uint8, got {tuple(t.shape)} {t.dtype}")
    return t


def resize_page_u8(page_u8, size, device=None):
    """``[H, W, 3]`` uint8 -> ``[hs, ws, 3]`` uint8 for ``size = (hs, ws)``, equal byte for byte to
    ``PIL.Image.resize((ws, hs), Image.BICUBIC)``, computed on the device.  numpy or torch in, the same kind (and device) out; a host
    page is computed on ``device`` (default ``cuda:0``).  A side may change by a factor of 8 at the most, either way."""
    t = _page_tensor(page_u8)
    hs, ws = int(size[0]), int(size[1])
    _check_resize(int(t.shape[0]), int(t.shape[1]), hs, ws)
    dev = torch.device(device) if device is not None else (t.device if t.is_cuda else torch.device("cuda:0"))
    out = _page_resize_u8(t.to(dev).contiguous(), hs, ws)
    if isinstance(page_u8, np.ndarray):
        return out.cpu().numpy()
    return out if out.device == page_u8.device else out.to(page_u8.device)


def _text_plane_up(text_s, g: TileGrid):
    """working-resolution text plane -> (text ``[g.h, g.w]`` of 0 / 1, core counts) on the page's grid ``g`` (``tsii_text_plane_up``)"""
    text = torch.empty((g.h, g.w), dtype=torch.uint8, device=text_s.device)
    counts = torch.empty((g.count,), dtype=torch.int32, device=text_s.device)
    _same_device(text_s, text, counts)
    call("tsii_text_plane_up", ptr(text_s), int(text_s.shape[0]), int(text_s.shape[1]), g.h, g.w, g.tile, g.halo, ptr(text), ptr(counts),
         _lib.stream())
    return text, counts


def logit_of(threshold) -> float:
    """float32 ``log(p / (1 - p))``: the logit threshold ``TextEraser`` hands to ``tsii_tiles_text_mask`` (0 at p = 0.5)."""
    return float(np.log(np.float32(threshold) / (np.float32(1.0) - np.float32(threshold)), dtype=np.float32))


@contextmanager
def _eval_mode(*nets):
    """``eval()`` for the call, every sub-module's ``training`` flag put back afterwards (also when the call raises)."""
    saved = [(m, m.training) for net in nets if isinstance(net, nn.Module) for m in net.modules()]
    for net in nets:
        if isinstance(net, nn.Module):
            net.eval()
    try:
        yield
    finally:
        for m, flag in saved:
            m.training = flag


# The names ``TextEraser._mark`` is called with, in the order a page passes them (those of the stages that are off are left out, and of
# each "a / b" pair the grid gives the first, ``pack``'s windows the second).  A mark closes the stage of its name, which began at the
# mark before it: a stage's time on the stream is the time between those two.  Three marks close no stage: "start" (nothing is enqueued
# yet), "joined" (the read-back tensor is formed; "counts_d2h" behind it is the copy alone) and "planned" (the host has selected the
# tiles or planned the windows and uploaded their small index tensors).
STAGE_MARKS = ("start", "upload", "resize", "page_tiles_norm", "segmenter", "tiles_text_mask", "plane_up", "regions", "blocks", "seeds", "geometry",
               "hulls", "balloon", "flat", "smooth", "tone", "crops", "joined", "counts_d2h", "planned", "page_tiles_fill", "page_windows_fill", "filler", "blend",
               "compose_page_u8", "compose_page_windows_u8", "download")


@dataclass
class PageState:
    """One page between the three phases of ``TextEraser._erase``.  ``g`` / ``gs``: the page's grid and the segmenter's (the same
    object without a working resolution); ``text``: the text plane on ``g``, ``text_s``: the segmenter's own (``text`` itself without a
    working resolution); ``src``: the page the filler and compose see (``page_d``, or what the flat, smooth and tone stages painted);
    ``both``: clean and mask in one buffer (one download), ``mask_u8`` its mask part; ``compose_mask``: the plane compose writes its
    mask to (``mask_u8``, or scratch where a stage wrote the page's mask already); ``read_back``: the one tensor the synchronisation
    copies; ``logits``: the segmenter's, kept for the seeds stage only (None without ``seed``)."""
    g: TileGrid
    gs: TileGrid
    page_d: torch.Tensor
    text: torch.Tensor
    text_s: torch.Tensor
    src: torch.Tensor
    both: torch.Tensor
    mask_u8: torch.Tensor
    compose_mask: torch.Tensor
    read_back: torch.Tensor
    logits: torch.Tensor = None


class TextEraser:
    """``clean_u8, mask_u8 = TextEraser(segmenter, filler, ...)(page_u8)``.

    ``segmenter``: callable ``x[N,3,T,T] -> logits[N,1,T,T]`` (``TextSegament``, ``XceptionTextSegment``); ``x`` is the page
    normalised with ``mean`` / ``std``, mirror-extended beyond the page edges, fp32 in channels-last memory.
    ``filler``: callable taking ONE argument, the pair ``(x[N,3,T,T], mask)``, and returning ``out[N,3,T,T]`` -- the calling
    convention of ``ImageFill`` / ``ImageFillOrigin`` / ``ImageFillOriginV2``.  ``x`` is ``page / 255 * mask`` (not normalised,
    as the inpainting data set feeds it), ``mask`` a 3-channel ``MaskParts`` over one ``[N,T,T]`` plane: 1 = keep, 0 = hole
    (text, or beyond the page edge).  Both are called under ``torch.no_grad()``; modules run in ``eval()`` mode for the call.

    ``tile`` (multiple of 32) and ``halo``: tiles of ``tile`` pixels a side step by ``tile - 2 * halo``, each owns that core and
    sees ``halo`` pixels of context around it.  ``threshold`` is the text probability (``sigmoid(logit) > threshold``), ``dilate``
    the side of the square the text is grown by (odd, 1..31).  Tiles without text in their core skip the filler
    (``skip_blank_tiles=False`` sends all of them); selected tiles go to it in row-major order, ``tile_batch`` at a time.

    ``min_area`` > 1 drops the connected text regions (``connectivity`` 4 or 8, measured after the dilation) of fewer pixels before
    anything else sees the text plane: they select no tile, are not painted over and are not in the returned mask.  ``regions=True``
    (or a ``min_area`` > 1) also leaves ``last_regions``: a dict of ``table`` (numpy int32 ``[n, 6]``: label, area, y0, x0, y1, x1 of
    the kept regions, at most ``max_regions`` rows), ``found``, ``kept`` and ``truncated``, read back with the tile counts in the
    page's one synchronisation; the int32 label plane stays on the device as ``last_labels``.  With the defaults none of this runs
    and both stay ``None``.

    ``hull=True`` (turns the regions path on as well) fills the convex hull of every kept region into the text plane right behind the
    filter, as the reference demo's ``cv2.convexHull`` + ``drawContours`` does: letter counters, the gaps between glyphs and dropped
    specks inside a text block become hole, so the filler gets one solid hole per block.  The returned mask, the tile selection, the
    filler's holes and ``last_stats["text_pixels"]`` all see the filled plane; ``last_regions`` gains ``hull_area`` (numpy int32, the
    pixels of each table row's hull).  Kept regions beyond ``max_regions`` get no hull.  Still one synchronisation.

    ``seg_long_side`` (a positive multiple of 8, like ``EvaluateSet.resize``): the segmenter sees the page resized to
    ``working_size(H, W, seg_long_side)`` -- long side ``seg_long_side``, both sides floored to a multiple of 8, Pillow's bicubic
    filter -- on that page's own tile grid; ``threshold`` and ``dilate`` act at that resolution, as in the reference, and the text
    plane is brought back to the page ("bilinear, then ``> 0``") before anything else sees it: ``min_area``, the returned mask and
    the filler work in page pixels.  A side of the page may be at most 8 x its working side (and the other way round).
    ``last_stats`` then also has ``seg_tiles`` and ``seg_size``.  ``None`` (the default): the page's own resolution, none of this runs.

    ``flat=T`` (an integer 0..255; turns the regions path on as well): a text region whose ring of surrounding page pixels -- those
    within ``flat_ring`` (1..8) pixels of it that are not text themselves -- is uniform within ``T`` grey levels in every channel is
    painted with the ring's mean colour on the device, right behind the filter (and the hulls; the filled plane is labelled once more
    for it, since hull pixels carry no label).  Such a region selects no tile, is no hole for the filler -- which sees the painted
    pixels as valid context -- and is not among the boxes ``pack`` places its windows on; a page whose text is all flat never calls the
    filler.  The returned mask still holds every region, flat or not.  ``last_stats`` gains ``flat_regions`` and ``flat_pixels``
    (``text_pixels`` stays the count of the returned mask), ``last_regions`` gains ``flat``: a dict of ``table`` (the labelled
    components the stage worked on: ``last_regions["table"]`` itself without ``hull``), ``is_flat``, ``colour`` (uint8 ``[n, 3]``) and
    ``ring_pixels``.  Regions without a ring and kept regions beyond ``max_regions`` are never flat.  Still one synchronisation.
    ``None`` (the default): none of this runs.

    ``smooth=T`` (an integer 0..255; turns the regions path on as well): the route between ``flat`` and the filler.  A text region is SMOOTH
    when no pixel of its ring -- ``smooth_ring`` (1..8) wide, as for ``flat`` -- differs from a neighbouring pixel that is not text by more
    than ``T`` grey levels in any channel: a gradient, a soft shadow or a sky passes, a hard edge or screentone across the region does
    not.  Such a region is filled with the harmonic continuation of the pixels around the page's text (``harmonic_fill`` on the whole
    page with ``smooth_sweeps`` sweeps: the same bytes), right behind the flat stage and on the page that stage painted; it selects no
    tile, is no hole for the filler -- which sees the filled pixels as valid context -- and is not among the boxes ``pack`` places its
    windows on; a page whose text is all flat or smooth never calls the filler.  The stage works on the labels and the table the flat
    stage works on (the second labelling behind ``hull`` is done once for both).  The returned mask still holds every region.
    ``last_stats`` gains ``smooth_regions`` and ``smooth_pixels``, ``last_regions`` gains ``smooth``: a dict of ``table``, ``is_smooth``,
    ``step`` (uint8 ``[n, 3]``: the largest step between neighbours in each ring) and ``ring_pixels``.  Still one synchronisation.
    ``None`` (the default): none of this runs.

    ``tone=T`` (an integer 0..255; turns the regions path on as well): the third route without a net, behind ``flat`` and ``smooth``.  A text
    region is TONE when its ring -- ``tone_ring`` (1..16) wide -- is textured (two neighbouring pixels differ by more than ``T`` somewhere)
    and repeats under one shift of 2..``tone_period`` (2..16) pixels along each axis: at least half the ring has a partner that is not
    text under the shift and no such pair differs by more than ``T`` grey levels in any channel.  Every pixel of such a region is filled
    with the nearest pixel that is not text a whole number of shifts away, on the page the earlier stages painted (what they filled is a
    valid source); the region selects no tile, is no hole for the filler and is not among the boxes ``pack`` places its windows on; a
    page whose text is all flat, smooth or tone never calls the filler.  The period must be a whole number of pixels at the page's
    resolution; the error is a maximum, so one outlier in the ring rejects a shift; there is one shift per region.  ``last_stats`` gains
    ``tone_regions`` and ``tone_pixels``, ``last_regions`` gains ``tone``: a dict of ``table``, ``is_tone``, ``shift`` (int32 ``[n, 2]``),
    ``err``, ``step`` and ``ring_pixels``.  Still one synchronisation.  ``None`` (the default): none of this runs.

    ``group=G`` (an integer 1..64; turns the regions path on as well): the connected regions are grouped into BLOCKS first -- two regions
    are in one block when some pixel of one is within ``G`` pixels (Chebyshev distance) of some pixel of the other, directly or through
    other regions: the lines of a speech bubble with a ``G`` of about the line spacing -- and everything behind works on blocks:
    ``min_area`` drops the blocks of fewer pixels (a dakuten beside its kana stays, a speck on its own goes), ``hull`` fills one hull
    per block (the gaps between glyphs and lines close), ``flat`` without ``hull`` judges the ring around the whole block, ``pack``
    plans its windows on the block boxes.  ``last_labels`` is then the block-label plane, ``last_regions["table"]`` the block table
    (``found`` / ``kept`` count blocks) with ``members`` (numpy int32, the regions in each row's block) and ``components`` (the regions
    of the page); ``last_stats`` gains ``blocks``.  Behind ``hull`` the flat stage labels the filled plane as before, ungrouped: hulls
    are solid.  Still one synchronisation.  ``None`` (the default): none of this runs.

    ``seed=P`` (a probability, ``threshold <= P < 1``; turns the regions path on as well): a hysteresis threshold.  ``threshold`` cuts low,
    so that faint and small lettering is caught; a region -- with ``group`` a block -- then stays only if at least ``min_seeds`` of its
    pixels have ``sigmoid(logit) > P`` (the seed plane: not dilated; with ``seg_long_side`` brought onto the page like the text plane, of
    which it is a subset).  The regions that do not are dropped on the device right behind ``min_area`` and the blocks, in front of
    everything else: they are not in the returned mask, select no tile, get no hull and no route, and ``pack`` plans no window on them.
    With ``group`` a faint mark beside a confident glyph stays, as a member of the glyph's block.  Kept regions beyond ``max_regions``
    are not judged and stay.  ``last_regions`` gains ``seeds`` (numpy int32, the seed pixels of each table row; ``table``, ``kept`` and
    ``members`` are those of the regions that stayed), ``last_stats`` gains ``seed_dropped`` and ``seed_dropped_pixels``.  Choose ``P`` with
    ``evaluate_eraser`` on raw / clean pairs: the mask's precision and recall with and without it.  Still one synchronisation.  ``None``
    (the default): none of this runs.

    ``geometry=True`` (turns the regions path on as well): every table row -- with ``group`` every block -- gets the polygon of its convex hull
    and its minimum-area enclosing rectangle, ``cv2.convexHull`` and ``cv2.minAreaRect`` in integers on the device: the oriented box a
    translation is typeset into, and the text angle.  The stage runs on ``last_labels`` and the table behind ``min_area``, the blocks and the
    seeds (dropped rows get no geometry) and in front of the hulls, which then fill the same polygons.  ``last_regions`` gains ``n_vertices``
    (numpy int32, the true count per row), ``vertices`` (int32 ``[n, max_vertices, 2]``: ``(y, x)`` from the top-left vertex clockwise, up to
    ``max_vertices`` 3..1024 of them) and ``rect`` (int64 ``[n, 8]``: ``k, dy, dx, lo_d, hi_d, lo_n, hi_n, D``, "K22" of
    ``include/tsii_hip.h``); ``RegionGeometry(None, n_vertices, vertices, rect)`` has the helpers ``polygon``, ``box_points``, ``size`` and
    ``angle``.  In page pixels, also behind ``seg_long_side``; sides up to 32767.  Still one synchronisation.  ``False`` (the default): none
    of this runs.

    ``crops=(ch, cw)`` (turns ``geometry`` on, and with it the regions path): rectified crops of the lettering.  Every kept table row's
    minimum-area rectangle -- with ``group`` every block's -- grown to cover its pixels' squares, is cut out of the RAW page on the device
    (the text is still in it), deskewed and scaled with its aspect ratio kept into the top-left corner of a slot of ``ch x cw`` pixels
    (sides 1..4096), the rest of the slot ``crop_fill`` (0..255): the batch an OCR net, a translation step or a review of what will be
    erased starts from, without a per-region loop on the host.  Bilinear in integers with up to ``crop_supersample`` (1..4) squared
    sub-samples per pixel where a block is reduced ("K23" of ``include/tsii_hip.h``): the same bits on every run.
    ``crop_orient="upright"`` turns a block by at most 45 degrees, so a vertical column stays tall; ``"long"`` lays the longer side along
    the slot's width, so a column reads rightwards, as a line recogniser wants it.  The stage runs behind the flat, smooth and tone stages
    on the geometry stage's rectangles: rows that ``seed`` or ``min_area`` dropped get no crop, nor do rows beyond ``max_crops``.  The
    slots stay on the device as ``last_crops`` (uint8 ``[max_crops, ch, cw, 3]``: ``max_crops * ch * cw * 3`` bytes, 2.4 MB at 64 slots of
    48 x 256; slots behind the rows served hold ``crop_fill``); ``last_regions`` gains ``crops``, a ``RegionCrops`` of the first ``n =
    min(rows, max_crops)`` slots and their ``info`` (numpy int32 ``[n, 10]``, which rides the one read-back as its last ``10 * max_crops``
    words) with the helpers ``crop``, ``quad``, ``to_page`` and ``scale``; ``last_stats`` gains ``crops = n``.  In page pixels, also
    behind ``seg_long_side``.  Still one synchronisation.  ``None`` (the default): none of this runs.

    ``balloon=T`` (an integer 0..255; turns the regions path on as well): where a translation has room.  For every table row -- with ``group``
    every block -- the ring within ``balloon_ring`` (1..8) pixels of the lettering gives a colour, as for ``flat``; where the ring is of one
    colour within ``T`` the BALLOON is the flood fill (4-connected) from the lettering over the page pixels within ``T`` of that colour that
    are no text, inside the row's box grown by ``balloon_reach`` (``balloon_ring``..512) pixels; other rows' lettering is an obstacle.  The
    stage runs on the RAW page and on the labels, the table and the text plane behind ``min_area``, the blocks, the seeds and the geometry,
    in front of the routes: the plane it reads holds every kept region and nothing has been painted ("K25" of ``include/tsii_hip.h``).  Its
    mark stands behind ``hulls``: with ``hull`` it reads a copy of the plane taken in front of the fill, so the hulls are no obstacle.
    ``last_regions`` gains ``balloons``, a ``RegionBalloons`` (``status``, ``is_balloon``, ``is_open``, ``colour``, ``ring_pixels``, ``area``,
    ``box``, ``anchor``, ``inner``: the largest upright rectangle inside the balloon around the block's centre, and ``rect``: the same in
    the layout ``region_crops`` takes); its 16 words per row ride the one read-back as the last ``16 * max_regions`` words.  ``last_stats``
    gains ``balloons`` and ``open_balloons``.  The rectangles stay on the device as ``last_balloon_rect`` (int64 ``[max_regions, 8]``), and
    ``typeset(page, slots, into="balloon")`` lays the slots into them instead of into the old lettering's footprint.  A row whose window
    would exceed 1024 pixels a side has no balloon (status bit 8).  In page pixels, also behind ``seg_long_side``.  Still one
    synchronisation.  ``None`` (the default): none of this runs.

    ``blend=True``: seamless (gradient-domain, Poisson) composition of what the filler paints.  An inpainting net reproduces structure well
    and absolute level badly: its patch is plausible and a shade lighter or darker than the page around it.  The filler returns the whole
    tile, so its error ``x - clamp(out, 0, 1)`` is known at the valid pixels around every hole; between the filler and compose the harmonic
    continuation of that error into the holes (``blend_sweeps`` 0..16 sweeps per level, the solver of ``HarmonicFill``) is added to the
    filler's clamped output there, on the device, for all tiles or windows in one call: the filler's gradients, the page's level --
    ``TextEraser(segmenter, SeamlessFill(filler, blend_sweeps))``, byte for byte, on the grid and with ``pack``.  A filler whose error is
    one constant comes back exact; ``HarmonicFill`` is left as it is (it has no error at the valid pixels).  The limits: the correction
    is per tile -- a hole across two cores is corrected by each tile from its own window, so the two halves may meet at slightly
    different levels; it interpolates the filler's error at the ring, so noise there is spread smoothly a few pixels into the hole; a
    tile without a valid pixel is not corrected.  Whether it helps a given checkpoint is for ``evaluate_eraser`` on raw / clean pairs to
    say (the ``fill`` and ``routes["net"]`` rows).  ``last_stats`` gains ``blended``, the tiles or windows that went through it.  Still one
    synchronisation.  ``False`` (the default): none of this runs.

    The page is ``[H, W, 3]`` uint8, numpy or torch, host or device, any ``H, W >= 1``; the results come back the same kind, on
    the same device.  A list of pages gives a list of ``(clean, mask)`` pairs.  ``mask`` is ``[H, W]`` uint8, 255 = text;
    ``clean`` equals the page wherever ``mask`` is 0.
    """

    def __init__(self, segmenter, filler, mean=(0.4935, 0.4563, 0.4544), std=(0.3769, 0.3615, 0.3566), tile=512, halo=64,
                 threshold=0.5, dilate=3, tile_batch=8, device=None, skip_blank_tiles=True, min_area=0, connectivity=8, regions=False,
                 max_regions=4096, seg_long_side=None, hull=False, pack=False, flat=None, flat_ring=3, group=None, smooth=None,
                 smooth_ring=3, smooth_sweeps=8, tone=None, tone_ring=8, tone_period=12, seed=None, min_seeds=1, blend=False, blend_sweeps=8,
                 geometry=False, max_vertices=64, crops=None, max_crops=64, crop_orient="upright", crop_fill=255, crop_supersample=4,
                 balloon=None, balloon_ring=3, balloon_reach=256):
        tile_grid(1, 1, tile, halo)                     # validates tile / halo
        if not 0.0 < float(threshold) < 1.0:
            raise ValueError(f"threshold {threshold} must be a probability in (0, 1)")
        if int(dilate) != dilate or not 1 <= dilate <= 31 or dilate % 2 == 0:
            raise ValueError(f"dilate {dilate} must be odd, 1..31")
        if int(tile_batch) < 1:
            raise ValueError("tile_batch >= 1")
        check_region_args(connectivity, min_area, max_regions)
        if seg_long_side is not None and (int(seg_long_side) != seg_long_side or seg_long_side < 8 or seg_long_side % 8):
            raise ValueError(f"seg_long_side {seg_long_side} must be a positive multiple of 8")
        self.seg_long_side = None if seg_long_side is None else int(seg_long_side)
        self.min_area, self.connectivity, self.max_regions = int(min_area), int(connectivity), int(max_regions)
        self.hull, self.pack = bool(hull), bool(pack)
        if self.pack and not skip_blank_tiles:
            raise ValueError("pack=True places the filler's windows on the text: it needs skip_blank_tiles=True")
        if flat is not None or flat_ring != 3:
            check_flat_args(0 if flat is None else flat, flat_ring)
        self.flat, self.flat_ring = None if flat is None else int(flat), int(flat_ring)
        if group is not None:
            check_block_args(group)
        self.group = None if group is None else int(group)
        if smooth is not None or smooth_ring != 3 or smooth_sweeps != 8:
            check_smooth_args(0 if smooth is None else smooth, smooth_ring, smooth_sweeps)
        self.smooth, self.smooth_ring, self.smooth_sweeps = None if smooth is None else int(smooth), int(smooth_ring), int(smooth_sweeps)
        if tone is not None or tone_ring != 8 or tone_period != 12:
            check_tone_args(0 if tone is None else tone, tone_ring, tone_period)
        self.tone, self.tone_ring, self.tone_period = None if tone is None else int(tone), int(tone_ring), int(tone_period)
        self.routes = self.flat is not None or self.smooth is not None or self.tone is not None
        if seed is not None and not float(threshold) <= float(seed) < 1.0:
            raise ValueError(f"seed {seed} must be a probability in [threshold, 1) = [{threshold}, 1)")
        check_seed_args(min_seeds)
        self.seed, self.min_seeds = None if seed is None else float(seed), int(min_seeds)
        self.seed_logit = None if seed is None else logit_of(seed)
        if blend or blend_sweeps != 8:
            check_sweeps(blend_sweeps)
        self.blend, self.blend_sweeps = bool(blend), int(blend_sweeps)
        if geometry or max_vertices != 64:
            check_geometry_args(max_vertices)
        if crops is not None or (max_crops, crop_orient, crop_fill, crop_supersample) != (64, "upright", 255, 4):
            check_crop_args((1, 1) if crops is None else crops, max_crops, crop_orient, crop_fill, crop_supersample)
        self.crops = None if crops is None else (int(crops[0]), int(crops[1]))
        self.max_crops, self.crop_orient, self.crop_fill, self.crop_supersample = int(max_crops), crop_orient, int(crop_fill), int(crop_supersample)
        self.geometry, self.max_vertices = bool(geometry) or self.crops is not None, int(max_vertices)
        if balloon is not None or (balloon_ring, balloon_reach) != (3, 256):
            check_balloon_args(0 if balloon is None else balloon, balloon_ring, balloon_reach)
        self.balloon, self.balloon_ring, self.balloon_reach = None if balloon is None else int(balloon), int(balloon_ring), int(balloon_reach)
        self.regions = (bool(regions) or self.min_area > 1 or self.hull or self.pack or self.group is not None or self.routes
                        or self.seed is not None or self.geometry or self.balloon is not None)
        self.segmenter, self.filler = segmenter, filler
        self.tile, self.halo, self.dilate, self.tile_batch = int(tile), int(halo), int(dilate), int(tile_batch)
        self.threshold, self.skip_blank_tiles = float(threshold), bool(skip_blank_tiles)
        mean32, std32 = np.asarray(mean, np.float32).reshape(3), np.asarray(std, np.float32).reshape(3)
        self.scale = np.float32(1.0) / (np.float32(255.0) * std32)                       # float32 throughout
        self.shift = -mean32 / std32
        self.logit_threshold = logit_of(threshold)
        if device is None:
            p = next(segmenter.parameters(), None) if isinstance(segmenter, nn.Module) else None
            device = p.device if p is not None else torch.device("cuda:0")
        self.device = torch.device(device)
        self.last_stats = None                          # of the latest page: the ``last_stats`` keys of the class docstring
        self.last_regions = None                        # its regions (regions path only): the ``last_regions`` keys of the class docstring
        self.last_labels = None                         # its int32 label plane, left on the device
        self.last_crops = None                          # its crops (``crops`` only): uint8 ``[max_crops, ch, cw, 3]``, left on the device
        self.last_crop_info = None                      # their info, int32 ``[max_crops * 10]``, and (``_crop_rows``) the word of the row count, left on the device: what ``typeset`` reads
        self._crop_rows = self._crop_page = None
        self.last_balloon_rect = None                   # its balloons' inner rectangles (``balloon`` only): int64 ``[max_regions, 8]``, and (``_balloon_rows``) the device pair of the row count, left on the device: what ``typeset(into="balloon")`` reads
        self._balloon_rows = None
        self.last_route_labels = None                   # the int32 label plane the flat, smooth and tone stages worked on, left on the device; None unless one of them is enabled

    # A page runs in three phases over one PageState: _enqueue, _read_back (the one synchronisation) and _finish with _download behind
    # it (a method of its own: _erase puts the nets' flags back in front of it).  They call _mark at every boundary of STAGE_MARKS;
    # tools/erase_bench.py replaces it by a recorder of events and so times the code the call runs.
    def _mark(self, name):
        """the page's course has reached the boundary ``name`` of ``STAGE_MARKS``: nothing to do"""

    def _upload(self, page):
        return _page_tensor(page).to(self.device).contiguous()

    def _segment(self, page_d, g):
        tiles = _page_tiles_norm(page_d, g, self.scale, self.shift)
        self._mark("page_tiles_norm")
        x = tiles.permute(0, 3, 1, 2)                   # [N,3,T,T] view in channels-last memory: to_nhwc() inside the nets is free
        logits = None
        for b0 in range(0, g.count, self.tile_batch):
            lb = self.segmenter(x[b0:b0 + self.tile_batch])
            n = min(self.tile_batch, g.count - b0)
            if tuple(lb.shape) != (n, 1, g.tile, g.tile):
                raise ValueError(f"segmenter returned {tuple(lb.shape)} for {n} tiles of {g.tile}")
            lb = lb.reshape(n, g.tile, g.tile)
            if n == g.count:                            # one batch: no gather copy
                logits = lb.float().contiguous()
            else:
                if logits is None:
                    logits = torch.empty((g.count, g.tile, g.tile), dtype=torch.float32, device=self.device)
                logits[b0:b0 + n].copy_(lb)             # bf16 logits (bf16 activation storage) are cast here, once
        return logits

    def _layout(self, g):
        """the page's read-back tensor: what rides where in it"""
        return ReadBack(g.count, self.max_regions, self.hull, self.group is not None, self.flat is not None, self.smooth is not None,
                        self.tone is not None, regions=self.regions, seeds=self.seed is not None,
                        geometry=self.max_vertices if self.geometry else 0, crops=self.max_crops if self.crops is not None else 0,
                        balloons=self.balloon is not None)

    def _route(self, name, src, text, g, labels, own, mask_u8):
        """the flat, smooth or tone stage: fill the regions it takes and take them out of the text plane in place -> the filled page (a new
        buffer; ``src``: the page, or the stage's before).  ``labels`` and ``own``: the labelling the stages work on and its tensor,
        ``[core counts | found, kept | table | the stages' rows]``, whose core counts are rewritten for the reduced plane.  ``mask_u8``: the
        plane that gets the mask of the whole plane on entry, None where an earlier stage wrote the page's already."""
        run, scalars = {"flat": (_flat_regions, (self.flat_ring, self.flat)),
                        "smooth": (_smooth_regions, (self.smooth_ring, self.smooth, self.smooth_sweeps)),
                        "tone": (_tone_regions, (self.tone_ring, self.tone_period, self.tone))}[name]
        lay = self._layout(g).routes
        painted = torch.empty_like(src)
        run(src, text, labels, own[lay.table], own[lay.n_regions], own[lay.rows(name)], self.max_regions, *scalars, painted, mask_u8, g,
            own[lay.counts])
        return painted

    def _run_filler(self, img, mplane, g):
        """fp32 NHWC tiles and their mask planes through the filler, ``tile_batch`` at a time -> its outputs, fp32 NHWC"""
        x = img.permute(0, 3, 1, 2)
        ns, out = int(img.shape[0]), None
        for b0 in range(0, ns, self.tile_batch):
            n = min(self.tile_batch, ns - b0)
            ob = self.filler((x[b0:b0 + n], MaskParts.from_plane(mplane[b0:b0 + n], 3)))
            if tuple(ob.shape) != (n, 3, g.tile, g.tile):
                raise ValueError(f"filler returned {tuple(ob.shape)} for {n} tiles of {g.tile}")
            if n == ns:
                out = to_nhwc(ob.float())
            else:
                if out is None:
                    out = torch.empty((ns, g.tile, g.tile, 3), dtype=torch.float32, device=self.device)
                out[b0:b0 + n].copy_(ob.permute(0, 2, 3, 1))
        return out

    def _plan(self, table, truncated, g, n_grid):
        """the windows to use instead of the grid's ``n_grid`` tiles -> (origins, rects) on the host, or None: stay on the grid"""
        if truncated or n_grid < 2:                     # regions beyond the table have no box; one tile cannot become fewer
            return None
        origins, rects = plan_fill_windows(table[:, 2:6], g.h, g.w, g.tile, g.halo)
        return (origins, rects) if 0 < len(origins) <= MAX_FILL_WINDOWS and len(origins) < n_grid else None

    def _enqueue(self, page) -> PageState:
        """phase 1: everything up to the one tensor the synchronisation copies, on the stream"""
        self._mark("start")
        page_d = seg_page = self._upload(page)
        self._mark("upload")
        h, w = int(page_d.shape[0]), int(page_d.shape[1])
        g = gs = tile_grid(h, w, self.tile, self.halo)
        if self.seg_long_side is not None:
            hs, ws = working_size(h, w, self.seg_long_side)
            _check_resize(h, w, hs, ws)
            if (hs, ws) != (h, w):
                gs = tile_grid(hs, ws, self.tile, self.halo)
                seg_page = _page_resize_u8(page_d, hs, ws)
                self._mark("resize")
        logits = self._segment(seg_page, gs)
        self._mark("segmenter")
        text, counts = _tiles_text_mask(logits, gs, self.logit_threshold, self.dilate)
        self._mark("tiles_text_mask")
        text_s = text
        if gs is not g:
            text, counts = _text_plane_up(text_s, g)
            self._mark("plane_up")
        off = (h * w * 3 + 15) // 16 * 16               # clean + mask in one buffer (one download); the kernels want both 4-byte aligned
        both = torch.empty((off + h * w,), dtype=torch.uint8, device=self.device)
        mask_u8 = both[off:].view(h, w)
        st = PageState(g, gs, page_d, text, text_s, page_d, both, mask_u8, mask_u8, counts, logits if self.seed is not None else None)
        if self.regions:
            self._enqueue_regions(st)
        self._mark("joined")
        return st

    def _enqueue_regions(self, st):
        """the regions path of phase 1, in place on ``st.text``: labelling, blocks, seeds, hulls and the flat, smooth and tone stages"""
        g, text, lay = st.g, st.text, self._layout(st.g)
        second = whole = geometry = info = balloons = None
        if self.group is None:
            self.last_labels, first = _text_regions(text, self.connectivity, self.min_area, self.max_regions, g, tail=lay.tail + lay.extra)
            if lay.seeded:                              # the seeds' room rides behind the first tensor
                whole, first = first, first[lay.first]
            self._mark("regions")
        else:                                           # every region is labelled and no table is made: the blocks stage filters
            labels, every = _text_regions(text, self.connectivity, 0, 0, g)
            self._mark("regions")
            self.last_labels, first, whole = _text_blocks(text, labels, every[lay.n_regions], self.group, self.min_area, self.max_regions, g,
                                                          tail=lay.tail, extra=lay.extra)
            self._mark("blocks")
        if lay.seeded:
            members, room = lay.seed_room(whole)
            _region_seeds(text, self.last_labels, self._seed_plane(st), first, room, self.max_regions, self.min_seeds, members, g)
            st.logits = None
            self._mark("seeds")
        if self.geometry:                               # of the labelled pixels, in front of the hulls: the fill then covers the same polygons
            geometry = _region_geometry(self.last_labels, first[lay.routes.table], first[lay.n_regions], self.max_regions, self.max_vertices)
            self._mark("geometry")
        plain = text                                    # the plane of every kept region, as the labelling left it
        if self.hull:
            if self.balloon is not None:                # the hulls fill the plane in place: the balloon stage behind them reads a copy of it as it is now
                plain = text.clone()
            _region_hulls(text, self.last_labels, first, self.max_regions, g)
            self._mark("hulls")
        if self.balloon is not None:                    # on the raw page and the plane of every kept region: nothing has been filled or painted there
            balloons, self.last_balloon_rect, _, _ = _region_balloons(st.page_d, plain, self.last_labels, first[lay.routes.table], first[lay.n_regions],
                                                                      self.max_regions, self.balloon_ring, self.balloon, self.balloon_reach)
            self._balloon_rows = first[lay.n_regions]
            self._mark("balloon")
        if self.routes:
            labels, own = self.last_labels, first
            if self.hull:                               # hull pixels carry no label: the filled plane is labelled once more, for all stages
                labels, own = _text_regions(text, self.connectivity, 0, self.max_regions, g, tail=lay.second_tail)
                second = own
            self.last_route_labels = labels
            for k, name in enumerate(lay.routes.stages):        # each works on the page the one before left
                st.src = self._route(name, st.src, text, g, labels, own, None if k else st.mask_u8)
                self._mark(name)
            st.compose_mask = torch.empty_like(st.mask_u8)      # the first stage wrote the page's mask; compose's, of the reduced plane, is scratch
        if self.crops is not None:                      # of the RAW page: the lettering is what is wanted; on the rectangles of the geometry stage
            self.last_crops, info = _region_crops(st.page_d, geometry[lay.geometry.rect], first[lay.n_regions], self.max_regions, self.crops,
                                                  self.max_crops, self.crop_orient, self.crop_fill, self.crop_supersample)
            self.last_crop_info, self._crop_rows, self._crop_page = info, first[lay.n_regions][1:], (g.h, g.w)
            self._mark("crops")
        st.read_back = lay.join(first, second, whole, geometry, info, balloons)

    def _seed_plane(self, st):
        """the seed plane on the page's grid: ``logit > logit_of(seed)``, not dilated, through the kernels that made the text plane"""
        seed, _ = _tiles_text_mask(st.logits, st.gs, self.seed_logit, 1)
        if st.gs is not st.g:
            seed, _ = _text_plane_up(seed, st.g)
        return seed

    def _read_back(self, st):
        """phase 2: the one synchronisation before the download -> ``regions.PageRead``"""
        host = st.read_back.cpu().numpy()
        self._mark("counts_d2h")
        read = self._layout(st.g).unpack(host)
        if self.regions:
            named = ("table", "found", "kept", "truncated", "members", "components", "hull_area", "seeds", "n_vertices", "vertices", "rect")
            self.last_regions = {k: getattr(read, k) for k in named if getattr(read, k) is not None}
            self.last_regions.update(read.stages)
            if read.crop_info is not None:
                self.last_regions["crops"] = RegionCrops(self.last_crops[:len(read.crop_info)], read.crop_info)
            if read.balloon_rows is not None:           # the rectangles are a function of the rows: nothing more is read back
                rect = balloon_rect_rows(read.balloon_rows)
                self.last_regions["balloons"] = RegionBalloons(None, read.balloon_rows, rect, None, read.table)
        return read

    def _finish(self, st, read):
        """phase 3, up to its download (``_download``): select or plan, fill, compose into ``st.both``; ``last_stats``"""
        g, h, w = st.g, st.g.h, st.g.w
        selected = [t for t in range(g.count) if read.counts[t] > 0 or not self.skip_blank_tiles]
        any_text = bool(read.counts.sum() > 0)
        windows = self._plan(read.plan_table, read.plan_truncated, g, len(selected)) if (self.pack and any_text) else None
        where = None                                    # on the device: (origin, rect) of the windows, or (ids, slot) of the grid's tiles
        if windows is not None:
            where = [torch.from_numpy(a).to(self.device) for a in windows]
        elif selected and any_text:
            slot_h = np.full(g.count, -1, np.int32)
            slot_h[selected] = np.arange(len(selected), dtype=np.int32)
            where = [torch.tensor(selected, dtype=torch.int32).to(self.device), torch.from_numpy(slot_h).to(self.device)]
        self._mark("planned")
        out = None
        if where is not None:
            img, mplane = (_page_tiles_fill if windows is None else _page_windows_fill)(st.src, st.text, g, where[0])
        self._mark("page_tiles_fill" if windows is None else "page_windows_fill")
        if where is not None:
            out = self._run_filler(img, mplane, g)
        self._mark("filler")
        if self.blend:                                  # the filler's error at the valid pixels, continued into the holes and added there
            if out is not None:
                out = _seamless_fill(img, out, mplane, self.blend_sweeps)
            self._mark("blend")
        clean = st.both[:h * w * 3].view(h, w, 3)
        if windows is None:
            _compose_page_u8(st.src, st.text, out, None if where is None else where[1], g, clean, st.compose_mask)
        else:
            _compose_page_windows_u8(st.src, st.text, out, *where, g, clean, st.compose_mask)
        self._mark("compose_page_u8" if windows is None else "compose_page_windows_u8")
        route_stats = {}                                # "flat_regions", "flat_pixels", ... of the enabled stages
        for name, stage in read.stages.items():
            route_stats[name + "_regions"] = int(stage["is_" + name].sum())
            route_stats[name + "_pixels"] = int(read.route_table[stage["is_" + name], 1].sum(dtype=np.int64))
        self.last_stats = {"tiles": g.count, "selected": int(out.shape[0]) if out is not None else 0,
                           "text_pixels": int(read.counts.sum()) + sum(v for k, v in route_stats.items() if k.endswith("_pixels"))}
        if self.group is not None:
            self.last_stats.update(blocks=read.kept)
        self.last_stats.update(route_stats)
        if self.blend:
            self.last_stats.update(blended=self.last_stats["selected"])
        if self.seed is not None:
            self.last_stats.update(seed_dropped=read.seed_dropped, seed_dropped_pixels=read.seed_dropped_pixels)
        if self.crops is not None:
            self.last_stats.update(crops=len(read.crop_info))
        if self.balloon is not None:
            b = self.last_regions["balloons"]
            self.last_stats.update(balloons=int(b.is_balloon.sum()), open_balloons=int((b.is_balloon & b.is_open).sum()))
        if self.pack:
            self.last_stats.update(packed=windows is not None, windows=self.last_stats["selected"],
                                   grid_selected=len(selected) if any_text else 0)
        if self.seg_long_side is not None:
            self.last_stats.update(seg_tiles=st.gs.count, seg_size=(st.gs.h, st.gs.w))

    def _download(self, st, page):
        """the end of phase 3: the one download -> (clean, mask) of the kind of ``page``, on its device"""
        h, w = st.g.h, st.g.w
        both = st.both.cpu().numpy() if isinstance(page, np.ndarray) else st.both.to(page.device)
        self._mark("download")
        return both[:h * w * 3].reshape(h, w, 3), both[both.shape[0] - h * w:].reshape(h, w)

    def _erase(self, page):
        with torch.no_grad(), _eval_mode(self.segmenter, self.filler):
            st = self._enqueue(page)
            self._finish(st, self._read_back(st))
        return self._download(st, page)                 # behind the with: the nets' flags are put back while the device still works

    def __call__(self, page):
        if isinstance(page, (list, tuple)):
            return [self._erase(p) for p in page]
        return self._erase(page)

    def typeset(self, page_u8, slots, supersample=4, into="block"):
        """Lay ``slots`` -- pictures drawn into the slots of the latest page's crops, ``[n <= max_crops, ch, cw, 4]`` uint8 straight RGBA, or
        ``[..., 3]``, which is opaque; numpy or torch, host or device -- onto ``page_u8`` (``[H, W, 3]`` uint8, normally the ``clean`` the call
        just returned) where the crops were cut out: the page with its new lettering.  ``page_u8`` is not modified; the result is a copy of
        the same kind, on the same device.  Row ``r`` goes where ``last_regions["crops"]`` says slot ``r`` came from, a later row over an
        earlier one, rows without a crop paste nothing and no slots give the copy; antialiased, with up to ``supersample`` (1..4) squared sub-samples per page pixel
        (``paste_crops``, "K24: region paste").  The ``info`` of the crops stage is still on the device: nothing is uploaded but the slots (and
        a host page), and nothing is read back.  A call of its own behind ``__call__``: the page's course is not touched.

        ``into="balloon"`` (needs ``balloon=T`` as well) lays slot ``r`` into the inner rectangle of row ``r``'s balloon instead, the room the
        page has for a translation: the ``info`` is derived at call time from ``last_balloon_rect`` on the device (``tsii_region_crops`` into a
        scratch batch, upright) and the paste runs with that; a row without a balloon pastes nothing."""
        if into not in ("block", "balloon"):
            raise ValueError(f"into {into!r} must be 'block' or 'balloon'")
        if self.crops is None:
            raise RuntimeError("typeset needs the crops stage: TextEraser(crops=(ch, cw))")
        if into == "balloon" and self.balloon is None:
            raise RuntimeError("typeset(into='balloon') needs the balloon stage: TextEraser(balloon=T)")
        if self.last_crop_info is None:
            raise RuntimeError("typeset needs a page: no page has been erased yet")
        p = _page_tensor(page_u8)
        sl = torch.from_numpy(np.ascontiguousarray(slots)) if isinstance(slots, np.ndarray) else slots
        if (not isinstance(sl, torch.Tensor) or sl.dtype != torch.uint8 or sl.dim() != 4 or sl.shape[0] > self.max_crops
                or tuple(sl.shape[1:3]) != self.crops or sl.shape[3] not in (3, 4)):
            raise ValueError(f"slots must be [0..{self.max_crops}, {self.crops[0]}, {self.crops[1]}, 3 or 4] uint8, got "
                             f"{tuple(sl.shape) if isinstance(sl, torch.Tensor) else type(sl)} {getattr(sl, 'dtype', '')}")
        _check_int_range("supersample", supersample, 1, 4)
        if tuple(p.shape[:2]) != self._crop_page:
            raise ValueError(f"page of {tuple(p.shape[:2])} pixels; the crops are those of a page of {self._crop_page}")
        out = p.to(self.device, copy=True).contiguous()
        if sl.shape[0] > 0 and into == "balloon":
            _, info = _region_crops(out, self.last_balloon_rect, self._balloon_rows, self.max_regions, self.crops, self.max_crops, "upright",
                                    self.crop_fill, 1)
            _region_paste(out, info, self._crop_rows, _rgba(sl.to(self.device)), supersample)
        elif sl.shape[0] > 0:                           # no slots: the copy, as paste_crops has it
            _region_paste(out, self.last_crop_info, self._crop_rows, _rgba(sl.to(self.device)), supersample)
        return out.cpu().numpy() if isinstance(page_u8, np.ndarray) else out.to(page_u8.device)

