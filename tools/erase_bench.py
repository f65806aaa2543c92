#!/usr/bin/env python3
"""Times one page through TextEraser stage by stage (HIP events on the launch stream) and prints one JSON line.

    python tools/erase_bench.py [--size 1170 1654] [--tile 512 --halo 64] [--repeats 10 --warmup 3] [--text-fraction 0.1]
                                [--min-area N [--connectivity 8]] [--hull] [--all-text] [--seg-long-side N] [--pack]
                                [--bubbles SHARE] [--flat T [--flat-ring N]] [--ramps SHARE] [--smooth T] [--tones SHARE] [--tone T [--tone-ring N] [--tone-period N]]
                                [--blend [--blend-sweeps N]] [--geometry [--max-vertices N]] [--balloon T [--balloon-ring N] [--balloon-reach N]]
                                [--crops HxW [--crop-orient long] [--max-crops N]]

Stages: upload, tsii_page_tiles_norm, segmenter, tsii_tiles_text_mask, counts read-back, tsii_page_tiles_fill, filler,
tsii_compose_page_u8, download.  The tool has no copy of the page's course: it puts a recorder in the place of ``TextEraser._mark``
(one HIP event per mark) and runs the eraser's own phases, ``_enqueue``, ``_read_back``, ``_finish`` and ``_download``; a stage's time
is the time between the mark that closes it and the mark before (``pipeline.STAGE_MARKS``).  So every stage is the code the call runs,
on the buffers the call uses: the ``segmenter`` stage includes the gather of the batches' logits, the ``filler`` stage is
``TextEraser._run_filler`` (the gather into one buffer instead of a list and ``torch.cat``), compose writes into the joint clean + mask
buffer and ``download`` is its one copy.  ``_segment`` is wrapped to put the synthetic logits in the net's place, ``_plan`` to time it
with the host clock.  Each kernel's bytes come from the accounting in DESIGN.md ("page pipeline"), computed here from
the shapes.  Random-init weights put no meaningful text on a page, so the segmenter's logits are timed as they are and then
REPLACED by a synthetic logit field (rectangular text blobs over ``--text-fraction`` of the page) for the stages behind it: what is
timed is the cost of the pipeline, not the quality of a net.  For comparison, in the same run:
* the mask stage the way examples/demo_segmentation.py does it (download the logits, threshold and nine torch.maximum on the CPU);
* a torch restatement of the tile, mask and compose stages on the device;
* the whole page with and without tile selection (pages / s, host clock around synchronised calls).
``--min-area N`` (N > 0) adds the ``regions`` stage (tsii_text_regions in place on the text plane, with the core counts) between the
mask and the read-back, which then carries the counts, the region counts and the table in its one copy; and ``host_route``, the same
labelling done the usual way: download the mask, scipy.ndimage.label + find_objects + bincount (reported as unavailable without
scipy).  ``--all-text`` makes the whole page one component: the worst case for the aggregation of areas and boxes.
``--hull`` adds the ``hulls`` stage (tsii_region_hulls in place on the text plane, right behind the regions stage, which it turns on),
and ``host_route_hulls``, the same step done the usual way: download the plane and the labels, ``scipy.spatial.ConvexHull`` per region,
``PIL.ImageDraw`` polygon fill, upload again (for timing only: a drawn polygon is not the hull's exact pixel set).
``--seg-long-side N`` runs the segmenter at the working size ``working_size(H, W, N)`` and adds the stages ``resize``
(tsii_page_resize_u8, between the upload and the tiles) and ``plane_up`` (tsii_text_plane_up, behind the mask); the synthetic text is
the same blob field, sampled at the working size.  ``host_route_resample`` times the same two steps the way the reference does them:
download the page, ``PIL.Image.resize(BICUBIC)``, upload; download the working mask, ``interpolate(bilinear) > 0``, upload.
``--pack`` (turns the regions stage on) places the filler's windows on the text regions: the host's ``plan_fill_windows`` is timed with
the host clock (``plan_host_ms``, behind the read-back, so nothing else is in flight), and where the windows are fewer than the grid's
tiles the stages ``page_tiles_fill`` / ``compose_page_u8`` are replaced by ``page_windows_fill`` / ``compose_page_windows_u8``
(tsii_page_windows_fill, tsii_compose_page_windows_u8); ``filler_tiles`` reports both counts.  Compare with a run without ``--pack`` in
the same session (same ``--min-area``).
``--bubbles SHARE`` replaces the page by a noisy one on which the first SHARE (0..1) of the blobs of the same blob field each sit on a
disc of one colour, as lettering sits in a speech bubble; ``--flat T`` (turns the regions stage on) adds the ``flat`` stage
(tsii_flat_regions, behind the regions / hulls stages; behind the hulls with the second labelling it needs, which is timed with it) and
sends the filler only what is left.  ``regions`` then reports ``flat_regions`` / ``flat_pixels`` and ``labelled`` (the components the
stage worked on).  Compare with a run on the same ``--bubbles`` page without ``--flat`` in the same session.

``--ramps SHARE`` is ``--bubbles`` with a linear colour ramp on every ellipse instead of one colour; ``--smooth T`` (turns the regions
stage on) adds the ``smooth`` stage (tsii_smooth_regions_classify, tsii_harmonic_fill on the whole page, tsii_smooth_regions_apply, behind
the flat stage; with its own pair of events, and, with the net as the filler, split into its three calls by events around each:
``smooth_split_ms``).  Compare with a run on the same ``--ramps`` page without ``--smooth`` in the same session.

``--tones SHARE`` is ``--bubbles`` with a dot lattice on every ellipse instead of one colour (period 6 along both axes, every other row of
dots offset by 3); ``--tone T`` (turns the regions stage on) adds the ``tone`` stage (tsii_tone_regions, behind the smooth stage) with its
own pair of events and reports the tone regions.  Compare with a run on the same ``--tones`` page without ``--tone`` in the same session.

``--group G`` (turns the regions stage on) adds the ``blocks`` stage (tsii_text_blocks, right behind the regions stage, which then labels
every region and leaves the filter to the blocks): its own pair of events.  ``regions`` then counts blocks in ``found`` / ``kept`` and
reports ``components`` and ``largest_block`` (members).  Compare with the same line without ``--group`` in the same session.

``--seed P`` (turns the regions stage on) adds the ``seeds`` stage (the seed plane by tsii_tiles_text_mask at dilate 1 -- and tsii_text_plane_up
with ``--seg-long-side`` -- then tsii_region_seeds, behind the regions / blocks stages) with its own pair of events; ``regions`` then reports
``seed_dropped`` / ``seed_dropped_pixels``.  ``--faint SHARE`` gives that share of the blobs a logit of 1 (a probability of 0.73) instead of
4, so that a ``P`` between the two has something to drop.  Compare with the same line without ``--seed`` in the same session.
``--geometry`` (turns the regions stage on) adds the ``geometry`` stage (tsii_region_geometry: hull polygons and minimum-area rectangles, behind
the regions / blocks / seeds stages) with its own pair of events; ``regions`` then reports ``hull_vertices`` and ``most_vertices``.  The stage
grows the read-back, so ``geometry_ab`` runs the whole page with and without it, alternating, in the same process: ``page_ms`` and the
``d2h_int32_words`` of both.
``--crops HxW`` (turns the geometry stage on) adds the ``crops`` stage (tsii_region_crops: every kept row's rectangle cut out of the raw page
into a slot of H x W pixels, behind the flat / smooth / tone stages) with its own pair of events; ``regions`` then reports ``crops`` (rows
served), ``crop_pixels`` (their pixels) and ``crop_subsamples`` (the bilinear samples behind them).  ``crops_ab`` runs the whole page with
and without it, alternating, in the same process, as ``geometry_ab`` does.
``--balloon T`` (turns the regions stage on; not to be confused with ``--bubbles``, which draws the page) adds the ``balloon`` stage
(tsii_region_balloons: per row the flood fill over the ring's colour, its area, box and open flag and the largest upright rectangle inside
it), timed between its marks; ``balloon_ab`` runs the whole page with and without it, alternating, in the same process, and reports the
read-back's growth and the sweeps the fill took per row (the debug words of the stage's workspace).
``--typeset`` (needs ``--crops``) times ``TextEraser.typeset`` behind the page, with the page's own crops as opaque slots: ``typeset`` reports
``call_ms`` (HIP events around the whole call on a device page: the copy of the page, the alpha plane and tsii_region_paste), ``kernels_ms``
(events around tsii_region_paste alone; compare with the ``crops`` stage of the same run), ``page_ms`` (the page on the host clock without and
with the call, alternating), ``rows`` (pasted), ``box_pixels`` (page pixels visited), ``subsamples`` and ``pixels_changed``.

``--blend`` adds the ``blend`` stage (tsii_seamless_fill on the filler's tiles or windows, between the filler and compose) with its own pair
of events.  Compare with the same line without ``--blend`` in the same session, and with ``--filler harmonic``, whose filler stage is the
stage's solver on the same tiles, ``tile_batch`` at a time and with the filler's gather.  ``blend_split_ms`` is the direct comparison: on
the tiles (or windows) the run sent, with their own hole planes, ``tsii_harmonic_fill`` alone and ``tsii_seamless_fill`` in one call each,
HIP events around the call: the difference is what the residual and apply passes add.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def blob_field(h, w, fraction, seed, rects=None, faint=0.0):
    """logits [h, w] of a page whose text is rectangular blobs covering about ``fraction`` of it (``rects``: a list that gets the blobs);
    ``faint``: this share of the blobs, evenly among them, has a logit of 1 instead of 4"""
    rng = np.random.default_rng(seed)
    page = np.full((h, w), -4.0, np.float32)
    target, covered, k = fraction * h * w, 0, 0
    while covered < target:
        bh, bw = int(rng.integers(30, 120)), int(rng.integers(60, 300))
        y, x = int(rng.integers(0, max(1, h - bh))), int(rng.integers(0, max(1, w - bw)))
        page[y:y + bh, x:x + bw] = 1.0 if (k % 10) < round(10 * faint) else 4.0
        k += 1
        covered += bh * bw
        if rects is not None:
            rects.append((y, x, bh, bw))
    return page


def bubble_page(h, w, rects, share, seed, margin=16, ramps=False, tones=False):
    """a noisy page; the first ``share`` of the blobs ``rects`` each on an ellipse of one colour that reaches ``margin`` pixels beyond the
    blob's corners (later bubbles may cut into earlier ones, blobs may touch: the share of FLAT regions is what the run reports).
    ``ramps``: every ellipse carries a linear colour ramp instead, 60 grey levels from end to end along a direction of its own.
    ``tones``: every ellipse carries a dot lattice instead: dots of 2 x 2 pixels 60 grey levels darker, period 6 along both axes, every
    other row of dots offset by 3 (the lattice vectors (3, 3) and (0, 6))."""
    rng = np.random.default_rng(seed)
    page = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    for y, x, bh, bw in rects[:int(round(share * len(rects)))]:
        ry, rx = (bh / 2 + margin) * 1.42, (bw / 2 + margin) * 1.42
        inside = ((yy - (y + bh / 2)) / ry) ** 2 + ((xx - (x + bw / 2)) / rx) ** 2 <= 1.0
        colour = rng.integers(180, 256, size=3, dtype=np.uint8)
        if tones:
            dots = ((yy % 6 < 2) & (xx % 6 < 2)) | (((yy + 3) % 6 < 2) & ((xx + 3) % 6 < 2))
            page[inside] = colour
            page[inside & dots] = colour - 60
            continue
        if not ramps:
            page[inside] = colour
            continue
        angle = rng.uniform(0.0, 2.0 * np.pi)
        along = ((yy - (y + bh / 2)) * np.sin(angle) + (xx - (x + bw / 2)) * np.cos(angle)) / max(ry, rx)      # -1 .. 1 across the ellipse
        page[inside] = np.clip(colour.astype(np.float64) - 30.0 + 30.0 * along[inside][:, None], 0, 255).astype(np.uint8)
    return page


def tile_logits(page, g, dev):
    """per-tile logits [nt, T, T] of the logit field ``page`` on the grid ``g``"""
    ext = np.pad(page, ((g.halo, g.ty * g.stride + g.halo), (g.halo, g.tx * g.stride + g.halo)), mode="edge")
    tiles = np.stack([ext[i * g.stride:i * g.stride + g.tile, j * g.stride:j * g.stride + g.tile]
                      for i in range(g.ty) for j in range(g.tx)])
    return torch.from_numpy(tiles).to(dev)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=(1170, 1654), metavar=("H", "W"))
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--halo", type=int, default=64)
    ap.add_argument("--dilate", type=int, default=3)
    ap.add_argument("--tile-batch", type=int, default=8)
    ap.add_argument("--seg-model", default="XceptionTextSegment")
    ap.add_argument("--fill-model", default="ImageFill")
    ap.add_argument("--text-fraction", type=float, default=0.1)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-area", type=int, default=0, help="> 0: time the regions stage with this filter")
    ap.add_argument("--connectivity", type=int, default=8, choices=[4, 8])
    ap.add_argument("--max-regions", type=int, default=4096)
    ap.add_argument("--hull", action="store_true", help="time the hulls stage (tsii_region_hulls) behind the regions stage")
    ap.add_argument("--geometry", action="store_true", help="time the geometry stage (tsii_region_geometry) behind the regions / blocks / seeds stages")
    ap.add_argument("--max-vertices", type=int, default=64, metavar="N", help="hull vertices read back per region with --geometry (3..1024)")
    ap.add_argument("--crops", default=None, metavar="HxW", help="time the crops stage (tsii_region_crops) into slots of H x W pixels; turns --geometry on")
    ap.add_argument("--crop-orient", default="upright", choices=["upright", "long"])
    ap.add_argument("--max-crops", type=int, default=64, metavar="N", help="slots with --crops")
    ap.add_argument("--balloon", type=int, default=None, metavar="T", help="time the balloon stage (tsii_region_balloons) at tolerance T (0..255)")
    ap.add_argument("--balloon-ring", type=int, default=3, metavar="N", help="ring width of the balloon stage (1..8)")
    ap.add_argument("--balloon-reach", type=int, default=256, metavar="N", help="pixels the balloon's window reaches beyond the block's box (ring..512)")
    ap.add_argument("--typeset", action="store_true", help="time TextEraser.typeset (tsii_region_paste) with the page's own crops as opaque slots; needs --crops")
    ap.add_argument("--all-text", action="store_true", help="the whole page is text: one component")
    ap.add_argument("--seg-long-side", type=int, default=None, help="segment at working_size(H, W, N); times the resize and plane_up stages")
    ap.add_argument("--pack", action="store_true", help="windows on the text regions instead of the grid's tiles (turns the regions stage on)")
    ap.add_argument("--bubbles", type=float, default=None, metavar="SHARE", help="a noisy page with this share of the blobs on discs of one colour")
    ap.add_argument("--flat", type=int, default=None, metavar="T", help="time the flat stage (tsii_flat_regions) with this tolerance")
    ap.add_argument("--flat-ring", type=int, default=3)
    ap.add_argument("--ramps", type=float, default=None, metavar="SHARE", help="--bubbles with a linear colour ramp on every ellipse")
    ap.add_argument("--smooth", type=int, default=None, metavar="T", help="time the smooth stage (tsii_smooth_regions_* around tsii_harmonic_fill) with this tolerance")
    ap.add_argument("--tones", type=float, default=None, metavar="SHARE", help="--bubbles with a dot lattice on every ellipse")
    ap.add_argument("--tone", type=int, default=None, metavar="T", help="time the tone stage (tsii_tone_regions) with this tolerance")
    ap.add_argument("--tone-ring", type=int, default=8)
    ap.add_argument("--tone-period", type=int, default=12)
    ap.add_argument("--group", type=int, default=None, metavar="G", help="time the blocks stage (tsii_text_blocks): regions within G pixels form a block")
    ap.add_argument("--seed", type=float, default=None, metavar="P", help="time the seeds stage (tsii_region_seeds): regions without a pixel above P are dropped")
    ap.add_argument("--min-seeds", type=int, default=1)
    ap.add_argument("--faint", type=float, default=0.0, metavar="SHARE", help="this share of the blobs has a logit of 1 instead of 4")
    ap.add_argument("--filler", default="net", choices=["net", "harmonic", "patch"], help="harmonic: T.HarmonicFill, patch: T.PatchFill in the filler stage; "
                    "no inpainting net is built")
    ap.add_argument("--sweeps", type=int, default=8, metavar="N", help="Jacobi sweeps per level of --filler harmonic and of the first guess of --filler patch (0..16)")
    ap.add_argument("--patch", type=int, default=7, metavar="N", help="window of --filler patch: odd, 3..9")
    ap.add_argument("--levels", type=int, default=4, metavar="N", help="pyramid levels of --filler patch (1..6)")
    ap.add_argument("--iters", type=int, default=4, metavar="N", help="search iterations per level of --filler patch (1..8)")
    ap.add_argument("--fill-seed", type=int, default=0, metavar="S", help="seed of the random search of --filler patch (32 bits)")
    ap.add_argument("--blend", action="store_true", help="time the blend stage (tsii_seamless_fill) between the filler and compose")
    ap.add_argument("--blend-sweeps", type=int, default=8, metavar="N", help="Jacobi sweeps per level of --blend (0..16)")
    args = ap.parse_args(argv)
    if args.typeset and args.crops is None:
        ap.error("--typeset needs --crops HxW")
    import text_segmentation_image_inpainting_amd as T
    from text_segmentation_image_inpainting_amd import pipeline as P
    from text_segmentation_image_inpainting_amd import regions as RG
    from text_segmentation_image_inpainting_amd.synthetic import manga_tile
    assert torch.cuda.is_available(), "erase_bench needs an MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    seg = getattr(T, args.seg_model)().to(dev).eval()
    if args.filler == "patch":
        fil = T.PatchFill(args.patch, args.levels, args.iters, args.fill_seed, args.sweeps)
    else:
        fil = T.HarmonicFill(args.sweeps) if args.filler == "harmonic" else getattr(T, args.fill_model)().to(dev).eval()
    h, w = args.size
    page = np.ascontiguousarray((manga_tile(max(h, w), np.random.default_rng(0)).transpose(1, 2, 0)[:h, :w] * 255).astype(np.uint8))
    g = gs = P.tile_grid(h, w, args.tile, args.halo)      # gs: the segmenter's grid
    hs, ws = (h, w) if args.seg_long_side is None else P.working_size(h, w, args.seg_long_side)
    if (hs, ws) != (h, w):
        gs = P.tile_grid(hs, ws, args.tile, args.halo)
    with_seg = gs is not g
    rects = []
    field = blob_field(h, w, 0.0 if args.all_text else args.text_fraction, 1, rects, args.faint)
    if args.bubbles is not None:
        page = bubble_page(h, w, rects, args.bubbles, 2)
    if args.ramps is not None:
        page = bubble_page(h, w, rects, args.ramps, 2, ramps=True)
    if args.tones is not None:
        page = bubble_page(h, w, rects, args.tones, 2, tones=True)
    if args.all_text:
        field.fill(4.0)
    if with_seg:                                          # the same text, sampled at the working size
        field = F.interpolate(torch.from_numpy(field)[None, None], size=(hs, ws), mode="nearest")[0, 0].numpy()
    logits_fixed = tile_logits(field, gs, dev)
    with_flat = args.flat is not None
    with_blocks = args.group is not None
    with_smooth = args.smooth is not None
    with_tone = args.tone is not None
    with_routes = with_flat or with_smooth or with_tone
    with_seeds = args.seed is not None
    crop_size = None if args.crops is None else tuple(int(v) for v in args.crops.lower().split("x"))
    args.geometry = args.geometry or crop_size is not None
    with_regions = args.min_area > 0 or args.hull or args.pack or with_blocks or with_routes or with_seeds or args.geometry or args.balloon is not None

    def make(select, geometry=args.geometry, crops=crop_size, balloon=args.balloon):
        er = T.TextEraser(seg, fil, tile=args.tile, halo=args.halo, dilate=args.dilate, tile_batch=args.tile_batch,
                          skip_blank_tiles=select, min_area=args.min_area, connectivity=args.connectivity, regions=with_regions,
                          max_regions=args.max_regions, seg_long_side=args.seg_long_side, hull=args.hull, pack=args.pack and select,
                          flat=args.flat, flat_ring=args.flat_ring, group=args.group, smooth=args.smooth, tone=args.tone,
                          tone_ring=args.tone_ring, tone_period=args.tone_period, seed=args.seed, min_seeds=args.min_seeds, blend=args.blend,
                          blend_sweeps=args.blend_sweeps, geometry=geometry, max_vertices=args.max_vertices, crops=crops,
                          max_crops=args.max_crops, crop_orient=args.crop_orient, balloon=balloon, balloon_ring=args.balloon_ring,
                          balloon_reach=args.balloon_reach)
        net = er._segment                                  # the segmenter runs and is timed; the blobs stand in for its logits
        er._segment = lambda page_d, grid: (net(page_d, grid), logits_fixed)[1]     # grid is gs: the eraser derives the same working size
        return er
    eraser = make(True)

    class Recorder:
        """``TextEraser._mark`` as a recorder: one HIP event per mark, on the current stream"""
        def __init__(self):
            self.names, self.events = [], []

        def __call__(self, name):
            self.names.append(name)
            self.events.append(torch.cuda.Event(enable_timing=True))
            self.events[-1].record()

        def stage_ms(self):
            """every mark but the first: the time from the mark before it (pipeline.STAGE_MARKS: the stage it closes)"""
            return {name: self.events[i].elapsed_time(self.events[i + 1]) for i, name in enumerate(self.names[1:])}

    planned, plan = {}, eraser._plan

    def timed_plan(*a):                                     # host clock: behind the read-back nothing else is in flight
        t0 = time.perf_counter()
        planned["windows"] = plan(*a)
        planned["ms"] = (time.perf_counter() - t0) * 1e3
        return planned["windows"]
    eraser._plan = timed_plan

    def one_page():
        rec = eraser._mark = Recorder()
        planned.update(windows=None, ms=0.0)
        with torch.no_grad():                               # the nets are in eval() mode already
            st = eraser._enqueue(page)
            read = eraser._read_back(st)                    # the one read-back: counts (+ region counts + table + flat rows + members)
            eraser._finish(st, read)
            eraser._download(st, page)
        torch.cuda.synchronize()
        stats, region_info = eraser.last_stats, None
        if with_regions:
            region_info = {"found": read.found, "kept": read.kept, "truncated": read.truncated}
            if with_blocks:
                region_info.update(components=read.components, largest_block=int(read.members.max()) if len(read.members) else 0)
            if with_seeds:
                region_info.update(seed_dropped=read.seed_dropped, seed_dropped_pixels=read.seed_dropped_pixels)
            if args.geometry:
                region_info.update(hull_vertices=int(read.n_vertices.sum(dtype=np.int64)), most_vertices=int(read.n_vertices.max()) if len(read.n_vertices) else 0)
            if crop_size is not None:
                ci = read.crop_info.astype(np.int64)
                region_info.update(crops=len(ci), crop_pixels=int((ci[:, 0] * ci[:, 1]).sum()), crop_subsamples=int((ci[:, 0] * ci[:, 1] * ci[:, 3] ** 2).sum()))
            if args.balloon is not None:
                b = eraser.last_regions["balloons"]
                region_info.update(balloons=stats["balloons"], open_balloons=stats["open_balloons"], balloon_pixels=int(b.area.sum(dtype=np.int64)),
                                   inner_pixels=int(((b.inner[:, 2] - b.inner[:, 0]) * (b.inner[:, 3] - b.inner[:, 1])).sum(dtype=np.int64)))
            if args.hull:
                region_info["hull_pixels"] = int(read.hull_area.sum(dtype=np.int64))
            if with_routes:
                region_info.update(labelled=len(read.route_table))
                region_info.update({name + s: stats[name + s] for name in read.stages for s in ("_regions", "_pixels")})
        return (rec.stage_ms(), int((read.counts > 0).sum()), int(read.counts.sum()), st, int(st.read_back.numel()), region_info,
                planned["windows"], planned["ms"], read.counts)

    for _ in range(args.warmup):
        one_page()
    split_names = ["tsii_smooth_regions_classify", "tsii_harmonic_fill", "tsii_smooth_regions_apply"]
    if with_smooth and args.filler == "net":                # event pairs around the three calls of the smooth stage (_lib.start_timing)
        from text_segmentation_image_inpainting_amd import _lib
        _lib.start_timing(split_names)
    runs = [one_page() for _ in range(args.repeats)]
    smooth_split = None
    if with_smooth and args.filler == "net":
        rec = _lib.stop_timing()
        smooth_split = {n: {"median": round(statistics.median(v[0] for v in rec[n]), 4), "min": round(min(v[0] for v in rec[n]), 4),
                            "max": round(max(v[0] for v in rec[n]), 4)} for n in split_names}
    n_sel, n_text, state, windows = runs[0][1], runs[0][2], runs[0][3], runs[0][6]
    n_fill = n_sel if windows is None else len(windows[0])
    stages = [s for s in runs[0][0] if s not in ("joined", "planned")]      # those two marks close no stage
    ms = {s: [r[0][s] for r in runs] for s in stages}
    med = {s: statistics.median(v) for s, v in ms.items()}

    # bytes each kernel has to move ("page pipeline")
    npx, tpx = h * w, args.tile * args.tile
    nsp = hs * ws
    bytes_ = {"page_tiles_norm": 3 * nsp + 12 * gs.count * tpx, "tiles_text_mask": 5 * nsp,
              "page_tiles_fill": 4 * npx * n_sel / g.count + 16 * n_sel * tpx, "compose_page_u8": 8 * npx + 12 * n_text}
    if windows is not None:                                 # DESIGN.md, "packed filler windows": 4 bytes read per window pixel on the page
        oy, ox = windows[0][:, 0].astype(np.int64), windows[0][:, 1].astype(np.int64)
        on_page = int(((np.minimum(oy + args.tile, h) - np.maximum(oy, 0)) * (np.minimum(ox + args.tile, w) - np.maximum(ox, 0))).sum())
        del bytes_["page_tiles_fill"], bytes_["compose_page_u8"]
        bytes_.update(page_windows_fill=4 * on_page + 16 * n_fill * tpx, compose_page_windows_u8=8 * npx + 12 * n_text)
    if with_seg:
        bytes_.update(resize=3 * npx + 3 * nsp, plane_up=nsp + npx)      # DESIGN.md, "working resolution"
    if with_regions:
        bytes_["regions"] = 18 * npx        # local 1 + 4, measure 4, filter 4 + 4 + 1 ("text regions"); seams and statistics on top
    if with_blocks:                         # DESIGN.md, "text blocks": pack 4, dilate 1, the labelling of the dilated plane 18, min 4 (+ runs),
        bytes_["blocks"] = 48 * npx         # name 4 + 4 + 4, measure 4, filter 4 + 4 + 1
    if with_seeds:                          # DESIGN.md, "seeded regions": the seed plane 4 + 1 (and its way up), count 1 (+ 4 on the seeds),
        bytes_["seeds"] = 15 * npx + (nsp + npx if with_seg else 0)     # filter 4 + 1 (+ stores where a region goes)
    if args.geometry:                       # DESIGN.md, "region geometry": extents 4 (labels); the pairs, the vertex lists and the outputs are small beside it
        bytes_["geometry"] = 4 * npx
    if crop_size is not None:               # DESIGN.md, "region crops": 12 page bytes per sub-sample (cached: neighbours share them), 3 out per slot pixel
        bytes_["crops"] = 12 * runs[0][5]["crop_subsamples"] + 3 * runs[0][5]["crops"] * crop_size[0] * crop_size[1]
    if args.hull:
        bytes_["hulls"] = 5 * npx + n_text  # extents 4 (labels), finish 1, the fill's stores at most once per final text pixel ("region hulls")
    if with_flat:                           # DESIGN.md, "flat regions": ring 1 (text) + apron, apply 3 + 1 in, 3 + 1 + 1 out, labels on the text
        apron = (64 + 2 * args.flat_ring) * (32 + 2 * args.flat_ring) / 2048.0
        bytes_["flat"] = int(apron * npx) + 9 * npx + 8 * int(runs[0][5]["flat_pixels"] + n_text) + (18 * npx if args.hull else 0)
    if with_smooth:                         # DESIGN.md, "smooth regions": stage 4 in + 16 out, ring 1 + 3 (+ aprons), the solver 2.1 x (12 + 4) in
        bytes_["smooth"] = 20 * npx + 4 * npx + int(2.1 * 16 * npx) + 12 * npx + 9 * npx      # + 12 out, apply 3 + 1 in, 3 + 1 + 1 out
    if with_tone:                           # DESIGN.md, "tone regions": ring 1 (text) + aprons per shift chunk, source 1 + 4, apply 3 + 1 in, 3 + 1 + 1 out
        chunks = -(-((args.tone_period + 1) * (2 * args.tone_period + 1)) // 128)
        apron = (64 + 2 * args.tone_ring) * (32 + 2 * args.tone_ring) / 2048.0
        bytes_["tone"] = int(chunks * apron * npx) + npx + 9 * npx + 16 * int(runs[0][5]["tone_pixels"] + n_text)
    if args.blend:                          # DESIGN.md, "seamless fill", per tile pixel: residual 12 + 12 + 4 in, 12 out; the solver 2.1 x (12 + 4) in
        bytes_["blend"] = int((40 + 2.1 * 16 + 12 + 40) * n_fill * tpx)     # + 12 out; apply 12 + 12 + 4 in, 12 out

    def timed(fn, sync=True):
        for _ in range(args.warmup):
            fn()
        vals = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            if sync:
                torch.cuda.synchronize()
            vals.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": round(statistics.median(vals), 4), "min_ms": round(min(vals), 4), "max_ms": round(max(vals), 4)}

    page_d, text, text_s = state.page_d, state.text, state.text_s
    # (a) the parent's route for the mask stage: the page's logits to the host, threshold + 3 x 3 max-pool with nine torch.maximum
    stitched = torch.randn(1, 1, h, w, device=dev)

    def demo_mask():
        m = (stitched > 0).cpu()
        p = F.pad(m.float(), (1, 1, 1, 1), value=0)
        o = torch.zeros_like(m, dtype=torch.float32)
        for dy in range(3):
            for dx in range(3):
                o = torch.maximum(o, p[..., dy:dy + h, dx:dx + w])
        return o.byte()

    # (b) torch restatements on the device
    iy = torch.from_numpy(np.stack([np.arange(t // g.tx * g.stride - g.halo, t // g.tx * g.stride - g.halo + g.tile) for t in range(g.count)])).to(dev)
    ix = torch.from_numpy(np.stack([np.arange(t % g.tx * g.stride - g.halo, t % g.tx * g.stride - g.halo + g.tile) for t in range(g.count)])).to(dev)

    def refl(v, n):
        p = 2 * (n - 1)
        v = torch.remainder(v, p)
        return torch.where(v < n, v, p - v)
    ry, rx = refl(iy, h), refl(ix, w)
    scale, shift = torch.from_numpy(eraser.scale).to(dev), torch.from_numpy(eraser.shift).to(dev)

    def torch_norm():
        return page_d[ry[:, :, None], rx[:, None, :]].float() * scale + shift

    def torch_mask():
        return F.max_pool2d((stitched > 0).float(), args.dilate, 1, args.dilate // 2).byte()

    filled = torch.rand(h, w, 3, device=dev)

    def torch_compose():
        return torch.where(text[..., None] > 0, torch.floor(filled.clamp(0, 1) * 255 + 0.5).byte(), page_d), text * 255

    host_resample = None
    if with_seg:
        from PIL import Image

        def host_resize():
            small = np.asarray(Image.fromarray(page_d.cpu().numpy()).resize((ws, hs), Image.BICUBIC))
            return torch.from_numpy(small).to(dev)

        def host_plane_up():
            up = F.interpolate(text_s.cpu()[None, None].float(), size=(h, w), mode="bilinear", align_corners=False) > 0
            return up[0, 0].to(torch.uint8).to(dev)
        host_resample = {"resize": timed(host_resize), "plane_up": timed(host_plane_up)}

    blend_split = None
    if args.blend and n_fill > 0:                           # the run's own tiles or windows: the solver alone against the whole call
        from text_segmentation_image_inpainting_amd.fill import _harmonic_fill, _seamless_fill
        if windows is None:
            ids = torch.tensor([t for t in range(g.count) if runs[0][8][t] > 0], dtype=torch.int32, device=dev)
            img, mplane = P._page_tiles_fill(state.src, state.text, g, ids)
        else:
            img, mplane = P._page_windows_fill(state.src, state.text, g, torch.from_numpy(windows[0]).to(dev))
        net_out = torch.rand_like(img) * 1.2 - 0.1

        def events_ms(fn):
            for _ in range(args.warmup):
                fn()
            vals = []
            for _ in range(args.repeats):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                vals.append(e0.elapsed_time(e1))
            return {"median": round(statistics.median(vals), 4), "min": round(min(vals), 4), "max": round(max(vals), 4)}
        blend_split = {"tiles": int(img.shape[0]), "harmonic_fill_alone": events_ms(lambda: _harmonic_fill(img, mplane, args.blend_sweeps)),
                       "seamless_fill": events_ms(lambda: _seamless_fill(img, net_out, mplane, args.blend_sweeps))}

    host_route = None
    if with_regions:
        text0, _ = P._tiles_text_mask(logits_fixed, g, eraser.logit_threshold, args.dilate)      # the plane before the filter
        try:
            from scipy import ndimage
            structure = np.ones((3, 3), np.int32) if args.connectivity == 8 else None

            def host_regions():
                m = text0.cpu().numpy()
                lab, n = ndimage.label(m, structure=structure)
                return ndimage.find_objects(lab), np.bincount(lab.reshape(-1), minlength=n + 1)
            host_route = timed(host_regions, sync=False)
        except ImportError:
            host_route = "not available: scipy is not installed"

    host_route_hulls = None
    if args.hull:
        text1, _ = P._tiles_text_mask(logits_fixed, g, eraser.logit_threshold, args.dilate)
        labels1, packed1 = RG._text_regions(text1, args.connectivity, args.min_area, args.max_regions, g)
        table1 = RG.ReadBack(g.count, args.max_regions).unpack(packed1.cpu().numpy()).table
        try:
            from PIL import Image, ImageDraw
            from scipy.spatial import ConvexHull, QhullError

            def host_hulls():
                m, lab = text1.cpu().numpy(), labels1.cpu().numpy()
                img = Image.fromarray(m * 255)
                draw = ImageDraw.Draw(img)
                for label, _, y0, x0, y1, x1 in table1:
                    ys, xs = np.nonzero(lab[y0:y1, x0:x1] == label)
                    pts = np.stack([xs + x0, ys + y0], axis=1)
                    try:
                        pts = pts[ConvexHull(pts).vertices]
                    except QhullError:                      # fewer than three points, or all on one line
                        pass
                    draw.polygon([tuple(int(v) for v in p_) for p_ in pts], fill=255) if len(pts) > 1 else draw.point(tuple(int(v) for v in pts[0]), fill=255)
                return torch.from_numpy(np.asarray(img) // 255).to(dev)
            host_route_hulls = timed(host_hulls)
        except ImportError:
            host_route_hulls = "not available: scipy or Pillow is not installed"

    geometry_ab = None
    if args.geometry:                                       # the same page with and without the stage, alternating, in this very process
        pair = {"with": make(True, True, None), "without": make(True, False, None)}
        vals, words = {k: [] for k in pair}, {}
        for i in range(args.warmup + args.repeats):
            for k, er in pair.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                er(page)
                torch.cuda.synchronize()
                if i >= args.warmup:
                    vals[k].append((time.perf_counter() - t0) * 1e3)
        for k, er in pair.items():
            with torch.no_grad():
                words[k] = int(er._enqueue(page).read_back.numel())
        geometry_ab = {"page_ms": {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in vals.items()},
                       "d2h_int32_words": words, "max_vertices": args.max_vertices}

    crops_ab = None
    if crop_size is not None:                               # the same page with and without the stage, alternating, in this very process
        pair = {"with": make(True), "without": make(True, crops=None)}
        vals, words = {k: [] for k in pair}, {}
        for i in range(args.warmup + args.repeats):
            for k, er in pair.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                er(page)
                torch.cuda.synchronize()
                if i >= args.warmup:
                    vals[k].append((time.perf_counter() - t0) * 1e3)
        for k, er in pair.items():
            with torch.no_grad():
                words[k] = int(er._enqueue(page).read_back.numel())
        crops_ab = {"page_ms": {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in vals.items()},
                    "d2h_int32_words": words, "slots": [args.max_crops, *crop_size], "orient": args.crop_orient}

    balloon_ab = None
    if args.balloon is not None:                            # the same page with and without the stage, alternating, in this very process
        pair = {"with": make(True), "without": make(True, balloon=None)}
        vals, words = {k: [] for k in pair}, {}
        for i in range(args.warmup + args.repeats):
            for k, er in pair.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                er(page)
                torch.cuda.synchronize()
                if i >= args.warmup:
                    vals[k].append((time.perf_counter() - t0) * 1e3)
        for k, er in pair.items():
            with torch.no_grad():
                words[k] = int(er._enqueue(page).read_back.numel())
        er = pair["with"]                                   # the sweeps per row: the debug words of the stage's workspace, read right behind a call
        with torch.no_grad():
            bst = er._enqueue(page)
            blay = er._layout(bst.g)
            bfirst = bst.read_back[blay.first]
            brows, _, _, sweeps = RG._region_balloons(bst.page_d, torch.where(er.last_labels != 0, 1, 0).to(torch.uint8), er.last_labels,
                                                     bfirst[blay.routes.table], bfirst[blay.n_regions], args.max_regions, args.balloon_ring, args.balloon,
                                                     args.balloon_reach)
            n_brows = min(int(bfirst[blay.n_regions][1]), args.max_regions)
            sweeps = sweeps[:n_brows].cpu().numpy()
            brows = brows.cpu().numpy().reshape(-1, 16)[:n_brows]
        swept = sweeps[(brows[:, 0] & 27) == 0]
        balloon_ab = {"page_ms": {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in vals.items()},
                      "d2h_int32_words": words, "tol": args.balloon, "ring": args.balloon_ring, "reach": args.balloon_reach, "rows": n_brows,
                      "sweeps": {"rows_filled": int(len(swept)), "min": int(swept.min()) if len(swept) else 0,
                                 "median": float(np.median(swept)) if len(swept) else 0.0, "max": int(swept.max()) if len(swept) else 0,
                                 "sum": int(swept.sum())}}

    typeset = None
    if args.typeset:                                        # the way back: the page's own crops, opaque, laid onto the cleaned page (tsii_region_paste)
        from text_segmentation_image_inpainting_amd import _lib
        er = make(True)
        clean_d = torch.from_numpy(er(page)[0]).to(dev)
        slots = er.last_crops
        events, host = [], {"with": [], "without": []}
        _lib.start_timing(["tsii_region_paste"])
        for i in range(args.warmup + args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out_d = er.typeset(clean_d, slots)              # a device page in: the copy of the page, the alpha plane and the two kernels
            e1.record()
            if i >= args.warmup:
                events.append((e0, e1))
        kernels = [v[0] for v in _lib.stop_timing()["tsii_region_paste"]][args.warmup:]
        call_ms = [a.elapsed_time(b) for a, b in events]
        for i in range(args.warmup + args.repeats):        # the page on the host clock without and with the call, alternating
            for k in ("without", "with"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                clean_h = er(page)[0]
                if k == "with":
                    er.typeset(clean_h, slots)
                torch.cuda.synchronize()
                if i >= args.warmup:
                    host[k].append((time.perf_counter() - t0) * 1e3)
        plan = RG._region_paste(clean_d.clone(), er.last_crop_info, er._crop_rows, RG._rgba(slots), 4).cpu().numpy()
        live = plan[plan[:, 0] != 0]
        box = (live[:, 3] - live[:, 1] + 1) * (live[:, 4] - live[:, 2] + 1)
        spread = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        typeset = {"call_ms": spread(call_ms), "kernels_ms": spread(kernels), "page_ms": {k: spread(v) for k, v in host.items()},
                   "rows": int(len(live)), "box_pixels": int(box.sum()), "subsamples": int((box * live[:, 5] ** 2).sum()),
                   "pixels_changed": int((out_d != clean_d).any(dim=-1).sum()), "slots": [args.max_crops, *crop_size]}

    result = {
        "tool": "erase_bench", "page": [h, w], "tile": args.tile, "halo": args.halo, "dilate": args.dilate, "tile_batch": args.tile_batch,
        "seg_model": args.seg_model, "fill_model": args.fill_model if args.filler == "net" else repr(fil), "filler": args.filler,
        "sweeps": args.sweeps if args.filler != "net" else None, "tiles": g.count, "selected_tiles": n_sel,
        "seg_long_side": args.seg_long_side, "seg_size": [hs, ws], "seg_tiles": gs.count, "host_route_resample": host_resample,
        "text_fraction": round(n_text / npx, 4), "repeats": args.repeats, "warmup": args.warmup,
        "stage_ms": {s: {"median": round(med[s], 4), "min": round(min(v), 4), "max": round(max(v), 4)} for s, v in ms.items()},
        "kernel_gb": {k: round(v / 1e9, 5) for k, v in bytes_.items()},
        "kernel_tb_per_s": {k: round(v / (med[k] * 1e-3) / 1e12, 3) for k, v in bytes_.items()},
        "kernels_share_of_nets": round(sum(med[k] for k in bytes_) / (med["segmenter"] + med["filler"]), 5),
        "all_text": args.all_text, "min_area": args.min_area, "connectivity": args.connectivity,
        # the stages that copy to the host before the download: still one, whatever it carries
        "d2h_before_download": {"stages": [s_ for s_ in stages if s_.endswith("_d2h")], "int32_words": runs[0][4]},
        "regions": runs[0][5], "host_route": host_route, "hull": args.hull, "host_route_hulls": host_route_hulls,
        "bubbles": args.bubbles, "flat": args.flat, "flat_ring": args.flat_ring if with_flat else None, "group": args.group,
        "seed": args.seed, "min_seeds": args.min_seeds if with_seeds else None, "faint": args.faint,
        "ramps": args.ramps, "smooth": args.smooth, "smooth_split_ms": smooth_split,
        "tones": args.tones, "tone": args.tone, "tone_ring": args.tone_ring if with_tone else None,
        "tone_period": args.tone_period if with_tone else None,
        "blend": args.blend, "blend_sweeps": args.blend_sweeps if args.blend else None, "blend_split_ms": blend_split,
        "geometry": args.geometry, "geometry_ab": geometry_ab, "crops": args.crops, "crops_ab": crops_ab, "typeset": typeset,
        "balloon": args.balloon, "balloon_ab": balloon_ab,
        "pack": args.pack, "packed": windows is not None, "filler_tiles": {"grid": n_sel, "sent": n_fill},
        "plan_host_ms": None if not args.pack else {"median": round(statistics.median(r[7] for r in runs), 4),
                                                    "min": round(min(r[7] for r in runs), 4), "max": round(max(r[7] for r in runs), 4)},
        "demo_route_mask_stage": timed(demo_mask, sync=False),
        "torch_on_device": {"page_tiles_norm": timed(torch_norm), "tiles_text_mask": timed(torch_mask), "compose_page_u8": timed(torch_compose)},
    }
    for name, select in (("with_selection", True), ("without_selection", False)):
        er = make(select)
        t = timed(lambda: er(page))
        result["pages_per_s_" + name] = {"median": round(1e3 / t["median_ms"], 2), "ms": t, "selected_tiles": er.last_stats["selected"]}
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
