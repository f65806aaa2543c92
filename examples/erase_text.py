#!/usr/bin/env python3
"""Remove the text from comic pages: segment -> mask -> inpaint (the reference README's road) with ``TextEraser``.
Pages of any size are tiled on the device; only the tiles that contain text go through the inpainting net.
Needs an MI355X (the models have no CPU path).

    python examples/erase_text.py --img-folder pages [--seg-checkpoint seg.pt] [--fill-checkpoint fill.pt] [--out-folder out]
    python examples/erase_text.py --synthetic            # seeded manga-like page, random-init weights

Writes ``<name>_clean.png`` and ``<name>_mask.png`` (255 = text) per page; ``--synthetic`` also writes the page itself.
``--min-area N`` drops the connected text regions of fewer than N pixels on the device before anything is inpainted; ``--boxes`` also
writes ``<name>_boxes.png``, the page with the boxes of the kept regions outlined.  ``--hull`` fills the convex hull of every kept region
into the mask on the device (the reference demo's ``cv2.convexHull`` step), so that the inpainting net gets one solid hole per text block.
``--group G`` groups the regions that lie within G pixels of one another into blocks on the device first (a G of about the line spacing
makes a speech bubble's lettering one block): ``--min-area``, ``--hull``, ``--flat`` and ``--pack`` then work per block and ``--boxes``
outlines the blocks, the boxes a translation would be typeset into.
``--seed P`` (a probability, ``--threshold`` <= P < 1) makes the cut a hysteresis threshold: ``--threshold`` may then be low enough to catch
faint and small lettering, and a region (with ``--group``: a block) stays text only if the segmenter gave at least ``--min-seeds N`` (default
1) of its pixels more than P; the others are dropped on the device before anything is inpainted.  ``examples/evaluate.py --task eraser``
scores a P on raw / clean pairs.
``--geometry`` gives every kept region (with ``--group``: every block) the polygon of its convex hull and its minimum-area rotated rectangle on
the device (``cv2.convexHull`` and ``cv2.minAreaRect`` in integers) and draws both into ``<name>_boxes.png``: the hull in green, the rectangle,
grown to cover the pixels' squares, in blue; ``--boxes`` adds the upright boxes in red.  ``--max-vertices N`` (3..1024, default 64) bounds
the polygon that is read back, not the rectangle.
``--crops HxW`` cuts every kept region's (with ``--group``: every block's) rotated rectangle out of the raw page on the device, deskewed and
scaled into a slot of H x W pixels, and writes the first ``--max-crops N`` (default 64) as ``<name>_crop_NN.png``: what an OCR or translation
step reads.  ``--crop-orient long`` lays vertical columns along the slot's width instead of keeping them upright.
``--balloon T`` finds every kept region's (with ``--group``: every block's) speech balloon on the device -- the flood fill from the lettering over
the colour around it, within T grey levels -- and draws its box and the largest upright rectangle inside it into ``<name>_boxes.png``;
``--typeset-demo --into balloon`` then lays the slots into those rectangles instead of into the old lettering's boxes.
``--typeset-demo`` (needs ``--crops``) is the way back: each crop's number is rendered with PIL's built-in font, black on a transparent slot,
and ``TextEraser.typeset`` lays the slots onto the cleaned page on the device, along the rectangles the crops came from: ``<name>_typeset.png``.
``--seg-long-side N`` (a multiple of 8; the reference's demo uses 600) lets the segmenter work on the page resized to a long side of N,
the scale it was trained at; the resize and the way back of the mask run on the device, the inpainting net keeps the page's pixels.
``--pack`` sends the inpainting net windows centred on the text regions instead of the grid's tiles, where that takes fewer of them: a
text block is then inpainted whole, in the middle of one window.
``--flat T`` (0..255) paints the text regions whose surroundings (``--flat-ring N`` pixels around them, default 3) are of one colour within
T grey levels -- lettering in a speech bubble -- with that colour on the device; only the text over artwork goes to the inpainting net.
``--smooth T`` (0..255) fills the text regions whose surroundings (``--smooth-ring N`` pixels around them, default 3) show no step of more
than T grey levels between neighbouring pixels -- lettering on a gradient, a soft shadow, a sky -- with the harmonic continuation of those
surroundings (``--smooth-sweeps N``, default 8), behind ``--flat``; text over screentone or artwork still goes to the inpainting net.
``--tone T`` (0..255) fills the text regions whose surroundings (``--tone-ring N`` pixels around them, default 8) are a pattern that repeats
under one shift of 2..``--tone-period N`` (default 12) pixels within T grey levels -- lettering on screentone, stripes, a dot lattice --
by copying the pixel a whole number of periods away, behind ``--smooth``.  The period must be a whole number of pixels.
``--filler harmonic`` needs no inpainting checkpoint: the holes take the smooth continuation of their surroundings (``T.HarmonicFill``,
``--sweeps N`` Jacobi sweeps per level, default 8), the right fill for text on a gradient, a soft shadow or a sky; no inpainting net is
built or loaded.
``--filler patch`` needs none either and continues what runs UNDER the text -- a panel border, an outline, hatching, screentone of any pitch
-- with the page's own pixels (``T.PatchFill``: every hole pixel is a copy of a pixel of its tile whose ``--patch N`` x N window, odd 3..9,
default 7, matches; ``--levels N`` pyramid levels, ``--iters N`` search iterations per level, ``--fill-seed S``; the first guess is the
harmonic fill with ``--sweeps``).  It cannot draw what the tile does not contain.
``--blend`` takes what the inpainting net paints into the page in the gradient domain (seamless, Poisson composition): the net's own error at
the pixels around every hole, continued harmonically into the hole (``--blend-sweeps N`` Jacobi sweeps per level, default 8) and added
there, so that a patch whose content is right and whose level is a shade off no longer stands out.  Per tile, on the device, between the
net and the page; ``examples/evaluate.py --task eraser --blend`` says on raw / clean pairs whether it helps a checkpoint.
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".webp")


def synthetic_page(h, w, seed=0):
    """a seeded manga-like page of h x w pixels cut from one square synthetic tile"""
    from text_segmentation_image_inpainting_amd.synthetic import manga_tile
    side = max(h, w)
    tile = manga_tile(side, np.random.default_rng(seed)).transpose(1, 2, 0)
    return np.ascontiguousarray((tile[:h, :w] * 255).astype(np.uint8))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--img-folder", default=None)
    ap.add_argument("--out-folder", default=None, help="default: next to the inputs (a temporary folder with --synthetic)")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--synthetic-size", type=int, nargs=2, default=(1170, 1654), metavar=("H", "W"))
    ap.add_argument("--seg-model", default="XceptionTextSegment", choices=["XceptionTextSegment", "TextSegament"])
    ap.add_argument("--fill-model", default="ImageFill", choices=["ImageFill", "ImageFillOrigin", "ImageFillOriginV2"])
    ap.add_argument("--seg-checkpoint", default=None)
    ap.add_argument("--fill-checkpoint", default=None)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--halo", type=int, default=64)
    ap.add_argument("--dilate", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--tile-batch", type=int, default=8)
    ap.add_argument("--min-area", type=int, default=0, help="drop text regions of fewer pixels (after the dilation)")
    ap.add_argument("--connectivity", type=int, default=8, choices=[4, 8])
    ap.add_argument("--boxes", action="store_true", help="also write <name>_boxes.png")
    ap.add_argument("--geometry", action="store_true", help="hull polygon and minimum-area rotated rectangle of every kept region, drawn into <name>_boxes.png")
    ap.add_argument("--max-vertices", type=int, default=64, metavar="N", help="hull vertices read back per region with --geometry (3..1024)")
    ap.add_argument("--crops", default=None, metavar="HxW", help="write every kept region's deskewed crop, fitted into H x W pixels, as <name>_crop_NN.png")
    ap.add_argument("--crop-orient", default="upright", choices=["upright", "long"], help="long: columns are laid along the crop's width")
    ap.add_argument("--max-crops", type=int, default=64, metavar="N", help="crops written per page with --crops")
    ap.add_argument("--typeset-demo", action="store_true", help="with --crops: paste each crop's number back onto the cleaned page, as <name>_typeset.png")
    ap.add_argument("--into", default="block", choices=["block", "balloon"], help="with --typeset-demo: lay the slots into the old lettering's box, or "
                    "into the free rectangle of its speech balloon (needs --balloon)")
    ap.add_argument("--balloon", type=int, default=None, metavar="T", help="find every region's speech balloon (the flood fill over the colour around it, "
                    "within T grey levels) and draw its box and its inner rectangle into <name>_boxes.png")
    ap.add_argument("--balloon-ring", type=int, default=3, metavar="N", help="width of the ring of surrounding pixels --balloon takes the colour from (1..8)")
    ap.add_argument("--balloon-reach", type=int, default=256, metavar="N", help="pixels a balloon may reach beyond its lettering's box (ring..512)")
    ap.add_argument("--hull", action="store_true", help="fill the convex hull of every kept text region into the mask")
    ap.add_argument("--seg-long-side", type=int, default=None, help="segment at this long side (multiple of 8), as EvaluateSet(resize=N)")
    ap.add_argument("--pack", action="store_true", help="inpaint windows centred on the text regions instead of the grid's tiles")
    ap.add_argument("--flat", type=int, default=None, metavar="T", help="paint text regions whose surroundings are uniform within T grey levels")
    ap.add_argument("--flat-ring", type=int, default=3, metavar="N", help="width of the ring of surrounding pixels --flat looks at (1..8)")
    ap.add_argument("--smooth", type=int, default=None, metavar="T", help="fill text regions harmonically whose surroundings step by at most T grey levels")
    ap.add_argument("--smooth-ring", type=int, default=3, metavar="N", help="width of the ring of surrounding pixels --smooth looks at (1..8)")
    ap.add_argument("--smooth-sweeps", type=int, default=8, metavar="N", help="Jacobi sweeps per level of the --smooth fill (0..16)")
    ap.add_argument("--tone", type=int, default=None, metavar="T", help="copy-fill text regions whose surroundings repeat under one shift within T grey levels")
    ap.add_argument("--tone-ring", type=int, default=8, metavar="N", help="width of the ring of surrounding pixels --tone looks at (1..16)")
    ap.add_argument("--tone-period", type=int, default=12, metavar="N", help="the longest period along each axis --tone looks for (2..16)")
    ap.add_argument("--group", type=int, default=None, metavar="G", help="group text regions within G pixels (1..64) into blocks: --min-area, --hull, "
                    "--flat and --pack then work per block, --boxes draws the block boxes")
    ap.add_argument("--seed", type=float, default=None, metavar="P", help="keep a text region only if some pixel of it has a text probability above P "
                    "(--threshold <= P < 1): a hysteresis threshold")
    ap.add_argument("--min-seeds", type=int, default=1, metavar="N", help="the pixels above --seed a region needs to stay")
    ap.add_argument("--filler", default="net", choices=["net", "harmonic", "patch"], help="harmonic: fill the holes with T.HarmonicFill, patch: with "
                    "T.PatchFill (copies of page pixels); neither needs an inpainting net")
    ap.add_argument("--sweeps", type=int, default=8, metavar="N", help="Jacobi sweeps per level of --filler harmonic and of the first guess of --filler patch (0..16)")
    ap.add_argument("--patch", type=int, default=7, metavar="N", help="window of --filler patch: odd, 3..9")
    ap.add_argument("--levels", type=int, default=4, metavar="N", help="pyramid levels of --filler patch (1..6)")
    ap.add_argument("--iters", type=int, default=4, metavar="N", help="search iterations per level of --filler patch (1..8)")
    ap.add_argument("--fill-seed", type=int, default=0, metavar="S", help="seed of the random search of --filler patch (32 bits)")
    ap.add_argument("--blend", action="store_true", help="seamless composition: correct the level of what the filler paints from its error around the holes")
    ap.add_argument("--blend-sweeps", type=int, default=8, metavar="N", help="Jacobi sweeps per level of --blend (0..16)")
    args = ap.parse_args(argv)
    if args.typeset_demo and args.crops is None:
        ap.error("--typeset-demo needs --crops HxW")
    if args.into == "balloon" and args.balloon is None:
        ap.error("--into balloon needs --balloon T")
    import text_segmentation_image_inpainting_amd as T
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    nets = []
    for name, ckpt in ((args.seg_model, args.seg_checkpoint), (args.fill_model, args.fill_checkpoint)):
        if len(nets) == 1 and args.filler != "net":                        # kernels, not a net: nothing to build or load
            nets.append(T.HarmonicFill(args.sweeps) if args.filler == "harmonic" else
                        T.PatchFill(args.patch, args.levels, args.iters, args.fill_seed, args.sweeps))
            break
        net = getattr(T, name)()
        if ckpt:
            net.load_state_dict(torch.load(ckpt, map_location="cpu"))      # the tolerant loader: reports and skips what does not fit
        nets.append(net.to(dev).eval())
    eraser = T.TextEraser(nets[0], nets[1], tile=args.tile, halo=args.halo, dilate=args.dilate, threshold=args.threshold,
                          tile_batch=args.tile_batch, min_area=args.min_area, connectivity=args.connectivity, regions=args.boxes,
                          seg_long_side=args.seg_long_side, hull=args.hull, pack=args.pack, flat=args.flat, flat_ring=args.flat_ring, group=args.group,
                          smooth=args.smooth, smooth_ring=args.smooth_ring, smooth_sweeps=args.smooth_sweeps, tone=args.tone, tone_ring=args.tone_ring,
                          tone_period=args.tone_period, seed=args.seed, min_seeds=args.min_seeds, blend=args.blend, blend_sweeps=args.blend_sweeps,
                          geometry=args.geometry, max_vertices=args.max_vertices,
                          crops=None if args.crops is None else tuple(int(v) for v in args.crops.lower().split("x")), max_crops=args.max_crops,
                          crop_orient=args.crop_orient, balloon=args.balloon, balloon_ring=args.balloon_ring, balloon_reach=args.balloon_reach)
    if args.synthetic or args.img_folder is None:
        out_folder = args.out_folder or tempfile.mkdtemp(prefix="tsii_erase_")
        os.makedirs(out_folder, exist_ok=True)
        page = synthetic_page(*args.synthetic_size)
        Image.fromarray(page).save(os.path.join(out_folder, "synthetic.png"))
        pages = [("synthetic", page)]
    else:
        out_folder = args.out_folder or args.img_folder
        os.makedirs(out_folder, exist_ok=True)
        names = sorted(f for f in os.listdir(args.img_folder) if f.lower().endswith(EXTENSIONS)
                       and not f.endswith(("_clean.png", "_mask.png", "_boxes.png", "_typeset.png")))
        pages = ((os.path.splitext(f)[0], np.asarray(Image.open(os.path.join(args.img_folder, f)).convert("RGB"))) for f in names)
    t0 = time.time()
    for name, page in pages:
        clean, mask = eraser(page)
        Image.fromarray(clean).save(os.path.join(out_folder, name + "_clean.png"))
        Image.fromarray(mask).save(os.path.join(out_folder, name + "_mask.png"))
        if args.crops is not None:
            found = eraser.last_regions["crops"]
            for r in range(len(found.info)):
                if found.info[r, 0]:
                    Image.fromarray(found.crop(r).cpu().numpy()).save(os.path.join(out_folder, "%s_crop_%02d.png" % (name, r)))
            print("%s: %d crops" % (name, len(found.info)))
            if args.typeset_demo and len(found.info):                       # each row's number, black on a transparent slot, onto the cleaned page
                from PIL import ImageDraw, ImageFont
                font = ImageFont.load_default()
                slots = np.zeros((len(found.info), *eraser.crops, 4), np.uint8)
                for r in range(len(found.info)):
                    uh, uw = int(found.info[r, 0]), int(found.info[r, 1])
                    if args.into == "balloon":                              # the slot is fitted to the balloon's rectangle, upright: draw into all of it
                        uh, uw = eraser.crops
                    if uh and uw:
                        label = Image.new("L", (uw, uh), 0)
                        ImageDraw.Draw(label).text((1, 0), "%d" % r, fill=255, font=font)
                        slots[r, :uh, :uw, 3] = np.asarray(label)           # the glyphs are the alpha plane; the colour stays black
                Image.fromarray(eraser.typeset(clean, slots, into=args.into)).save(os.path.join(out_folder, name + "_typeset.png"))
        if args.boxes or args.geometry or args.balloon is not None:
            from PIL import ImageDraw
            boxed = Image.fromarray(page)
            draw = ImageDraw.Draw(boxed)
            if args.boxes:
                for _, _, y0, x0, y1, x1 in eraser.last_regions["table"].tolist():
                    draw.rectangle([x0, y0, x1 - 1, y1 - 1], outline=(255, 0, 0))
            if args.geometry:
                geo = T.RegionGeometry(None, *(eraser.last_regions[k] for k in ("n_vertices", "vertices", "rect")))
                for r in range(len(geo.n_vertices)):
                    for points, colour in ((geo.polygon(r), (0, 160, 0)), (geo.box_points(r, pad=True), (0, 0, 255))):
                        xy = [(float(x), float(y)) for y, x in points]
                        draw.line(xy + xy[:1], fill=colour)
                print("%s: %d oriented boxes, %d of them turned by more than 5 degrees" %
                      (name, len(geo.n_vertices), sum(5.0 < abs(geo.angle(r)) < 85.0 for r in range(len(geo.n_vertices)))))
            if args.balloon is not None:                                   # the balloon's box (orange; dashed-looking where open) and the room inside it (magenta)
                found = eraser.last_regions["balloons"]
                for r in np.nonzero(found.is_balloon)[0]:
                    (by0, bx0, by1, bx1), (ry0, rx0, ry1, rx1) = found.box[r].tolist(), found.inner[r].tolist()
                    draw.rectangle([bx0, by0, bx1 - 1, by1 - 1], outline=(255, 200, 120) if found.is_open[r] else (255, 140, 0))
                    draw.rectangle([rx0, ry0, rx1 - 1, ry1 - 1], outline=(255, 0, 255))
                print("%s: %d balloons, %d of them open" % (name, eraser.last_stats["balloons"], eraser.last_stats["open_balloons"]))
            boxed.save(os.path.join(out_folder, name + "_boxes.png"))
        if args.boxes:
            if args.group is not None:
                print("%s: %d text regions in %d blocks, %d kept" % (name, eraser.last_regions["components"], eraser.last_regions["found"],
                                                                     eraser.last_regions["kept"]))
            else:
                print("%s: %d text regions, %d kept" % (name, eraser.last_regions["found"], eraser.last_regions["kept"]))
        st = eraser.last_stats
        print("%s: %d x %d, %d of %d tiles inpainted, text fraction %.4f" %
              (name, page.shape[0], page.shape[1], st["selected"], st["tiles"], float((mask > 0).mean())))
        if args.seed is not None:
            print("%s: %d text regions (%d pixels) without a pixel above %g dropped" % (name, st["seed_dropped"], st["seed_dropped_pixels"], args.seed))
        if args.pack:
            print("%s: %s, the grid would have sent %d tiles" % (name, "%d windows on the text regions" % st["windows"] if st["packed"]
                                                                  else "no fewer windows than tiles: the grid's tiles", st["grid_selected"]))
        if args.flat is not None:
            print("%s: %d flat text regions (%d pixels) painted without the inpainting net" % (name, st["flat_regions"], st["flat_pixels"]))
        if args.smooth is not None:
            print("%s: %d smooth text regions (%d pixels) filled harmonically without the inpainting net" % (name, st["smooth_regions"], st["smooth_pixels"]))
        if args.tone is not None:
            print("%s: %d tone text regions (%d pixels) filled from one period away without the inpainting net" % (name, st["tone_regions"], st["tone_pixels"]))
        if args.blend:
            print("%s: %d tiles or windows blended into the page" % (name, st["blended"]))
        if "seg_size" in st:
            print("%s: segmented at %d x %d (%d tiles)" % ((name,) + tuple(st["seg_size"]) + (st["seg_tiles"],)))
    print("Runtime :{:.3f} s -> {}".format(time.time() - t0, out_folder))


if __name__ == "__main__":
    main()
