#!/usr/bin/env python3
"""Validate a checkpoint on the device: precision / recall / F1 / IoU over a threshold sweep for a segmentation net, L1 / PSNR /
SSIM for an inpainting net, and -- for the page pipeline that people run -- the score of a ``TextEraser`` over pairs of a raw page and the
same page cleaned by hand.  The metrics are accumulated by the kernels of ``csrc/metrics.hip`` and ``csrc/score.hip``; the host reads one
small result.  Needs an MI355X (the models have no CPU path).  Prints ONE JSON line.

    python examples/evaluate.py --task segmentation --img-folder train/raw [--checkpoint seg.pt] [--thresholds 19]
    python examples/evaluate.py --task inpainting --img-folder clean_pages [--checkpoint fill.pt]
    python examples/evaluate.py --task segmentation --synthetic 8          # seeded synthetic batches, random-init weights
    python examples/evaluate.py --task eraser --raw-folder raw --clean-folder clean [--flat 8 --tone 8 ...]
    python examples/evaluate.py --task eraser --synthetic 2 --flat 8       # seeded pages with dark lettering, random-init weights

Folders are what ``TextSegmentationData`` / ``ImageInpaintingData`` take.  For segmentation the line carries the sweep and
``suggested_eraser_threshold``: the probability with the best F1, to be passed as ``TextEraser(threshold=...)``.
``--task eraser`` pairs the files of the two folders by name (without the extension) and takes the eraser switches of
``examples/erase_text.py`` (``--tile``, ``--min-area``, ``--hull``, ``--group``, ``--seed``, ``--flat``, ``--smooth``, ``--tone``, ``--filler`` ...); the
truth mask comes from each pair as the reference's ``Dataloader`` derives it (``--brightness-difference``, ``--truth-dilate``).  The line
carries ``mask`` (precision / recall / F1 / IoU of the eraser's mask), ``fill`` and ``leftover`` (the error where the eraser painted and
where it did not) and ``routes``: per route -- ``flat``, ``smooth``, ``tone``, ``net`` -- the regions it took and how well it repaired them.
With ``--seed P`` (and ``--min-seeds N``) the same pairs are also run through the same eraser WITHOUT the seed, and the line gains
``without_seed``: that run's ``mask``, so that the precision bought and the recall paid for a P stand side by side; ``seed_dropped`` /
``seed_dropped_pixels`` are the regions the seed took out, over all pages.
With ``--blend`` (and ``--blend-sweeps N``) the filler's output is taken into the page in the gradient domain, the same pairs are also run
through the same eraser WITHOUT the blend, and the line gains ``without_blend``: that run's ``fill`` and ``routes``, so that what the blend
does to the painted pixels stands side by side; ``fill`` and ``routes["net"]`` are the rows to read.
The eraser's line is strict JSON: a ratio over nothing (a route that took no region) is ``null``, the PSNR of an error of zero ``"inf"``.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def synthetic_batches(task, images, batch, size):
    from text_segmentation_image_inpainting_amd import synthetic
    make = synthetic.make_seg_batch if task == "segmentation" else synthetic.make_batch
    for b0 in range(0, images, batch):
        yield make(min(batch, images - b0), size, seed0=1000 + b0)


def folder_batches(task, folder, batch, size):
    from torch.utils.data import DataLoader
    from text_segmentation_image_inpainting_amd import Dataloader
    if task == "segmentation":
        data = Dataloader.TextSegmentationData(folder, image_size=(size, size))
    else:
        data = Dataloader.ImageInpaintingData(folder, image_size=(size, size), add_random_masks=True)
    for items in DataLoader(data, batch_size=batch, shuffle=False):
        if task == "segmentation" and items[0].shape[1] == 1:
            items = (items[0].expand(-1, 3, -1, -1), items[1])
        yield tuple(items)


EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".webp")


def synthetic_pairs(pages, h, w):
    """seeded (raw, clean) pairs: a manga-like page, and the same page with rows of dark strokes drawn over it"""
    import numpy as np
    from examples.erase_text import synthetic_page
    for k in range(pages):
        clean = synthetic_page(h, w, seed=1000 + k)
        rng = np.random.default_rng(2000 + k)
        raw = clean.copy()
        for _ in range(max(6, h * w // 40000)):          # a block of lettering: 4 lines of strokes
            y0, x0 = int(rng.integers(0, max(h - 60, 1))), int(rng.integers(0, max(w - 120, 1)))
            for line in range(4):
                for stroke in range(12):
                    y, x = y0 + 14 * line, x0 + 9 * stroke
                    raw[y:y + 9, x:x + int(rng.integers(2, 7))] = rng.integers(0, 40, size=3)
        yield raw, clean


def folder_pairs(raw_folder, clean_folder):
    """(raw, clean) of every file name (without the extension) the two folders share, in sorted order"""
    import numpy as np
    from PIL import Image
    stems = lambda d: {os.path.splitext(f)[0]: os.path.join(d, f) for f in sorted(os.listdir(d)) if f.lower().endswith(EXTENSIONS)}
    raw, clean = stems(raw_folder), stems(clean_folder)
    names = sorted(set(raw) & set(clean))
    if not names:
        raise SystemExit(f"no file name in both {raw_folder} and {clean_folder}")
    for name in names:
        a, b = (np.asarray(Image.open(p[name]).convert("RGB")) for p in (raw, clean))
        if a.shape != b.shape:
            raise SystemExit(f"{name}: the raw page is {a.shape[:2]}, the clean page {b.shape[:2]}")
        yield a, b


def strict_json(value):
    """the eraser's line in strict JSON: a ratio that does not exist (a route without regions: nan) becomes null, the PSNR of an error of
    zero (inf) the string "inf"; a plain parser reads the line"""
    import math
    if isinstance(value, dict):
        return {k: strict_json(v) for k, v in value.items()}
    if isinstance(value, (list, tuple)):
        return [strict_json(v) for v in value]
    if isinstance(value, float) and not math.isfinite(value):
        return None if math.isnan(value) else ("inf" if value > 0 else "-inf")
    return value


def eraser_main(args):
    import text_segmentation_image_inpainting_amd as T
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    seg = getattr(T, args.seg_model)()
    if args.seg_checkpoint:
        seg.load_state_dict(torch.load(args.seg_checkpoint, map_location="cpu"))
    if args.filler == "harmonic":
        fill = T.HarmonicFill(args.sweeps)
    elif args.filler == "patch":
        fill = T.PatchFill(args.patch, args.levels, args.iters, args.fill_seed, args.sweeps)
    else:
        fill = getattr(T, args.fill_model)()
        if args.fill_checkpoint:
            fill.load_state_dict(torch.load(args.fill_checkpoint, map_location="cpu"))
        fill = fill.to(dev).eval()
    seg = seg.to(dev).eval()

    class Counting(T.TextEraser):
        """sums what the seed dropped over the pages"""
        dropped = dropped_pixels = 0

        def __call__(self, page):
            out = super().__call__(page)
            self.dropped += self.last_stats.get("seed_dropped", 0)
            self.dropped_pixels += self.last_stats.get("seed_dropped_pixels", 0)
            return out

    def make(seed, blend=args.blend):
        return Counting(seg, fill, tile=args.tile, halo=args.halo, dilate=args.dilate, threshold=args.threshold,
                        tile_batch=args.tile_batch, min_area=args.min_area, connectivity=args.connectivity, seg_long_side=args.seg_long_side,
                        hull=args.hull, pack=args.pack, flat=args.flat, flat_ring=args.flat_ring, group=args.group, smooth=args.smooth,
                        smooth_ring=args.smooth_ring, smooth_sweeps=args.smooth_sweeps, tone=args.tone, tone_ring=args.tone_ring,
                        tone_period=args.tone_period, seed=seed, min_seeds=args.min_seeds, blend=blend, blend_sweeps=args.blend_sweeps)
    make_pairs = lambda: synthetic_pairs(args.synthetic, *args.synthetic_size) if args.synthetic else folder_pairs(args.raw_folder, args.clean_folder)
    eraser = make(args.seed)
    res = T.evaluate_eraser(eraser, make_pairs(), T.EraserMetrics(args.brightness_difference, args.truth_dilate, ssim=args.ssim))
    if args.seed is not None:
        plain = T.evaluate_eraser(make(None), make_pairs(), T.EraserMetrics(args.brightness_difference, args.truth_dilate))
        res.update(seed=args.seed, min_seeds=args.min_seeds, seed_dropped=eraser.dropped, seed_dropped_pixels=eraser.dropped_pixels,
                   without_seed=plain["mask"])
    if args.blend:
        plain = T.evaluate_eraser(make(args.seed, blend=False), make_pairs(), T.EraserMetrics(args.brightness_difference, args.truth_dilate))
        res.update(blend=True, blend_sweeps=args.blend_sweeps, without_blend={"fill": plain["fill"], "routes": plain["routes"]})
    pages = [dict(sums=[int(v) for v in p["page"]], regions=len(p["rows"]), **({"ssim": p["ssim"]} if "ssim" in p else {})) for p in res.pop("pages")]
    line = {"task": "eraser", "seg_model": args.seg_model, "fill_model": {"harmonic": "HarmonicFill", "patch": repr(fill)}.get(args.filler, args.fill_model),
            "pages": len(pages), **res, "per_page": pages}
    line = strict_json(line)
    print(json.dumps(line, allow_nan=False))
    return line


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--task", required=True, choices=["segmentation", "inpainting", "eraser"])
    ap.add_argument("--img-folder", default=None)
    ap.add_argument("--raw-folder", default=None, help="eraser: the raw pages")
    ap.add_argument("--clean-folder", default=None, help="eraser: the same pages cleaned by hand, under the same file names")
    ap.add_argument("--synthetic-size", type=int, nargs=2, default=(600, 800), metavar=("H", "W"), help="eraser: the size of the --synthetic pages")
    ap.add_argument("--brightness-difference", type=float, default=0.4, help="eraser: the threshold of the pair's truth mask (Dataloader's)")
    ap.add_argument("--truth-dilate", type=int, default=10, help="eraser: the side of the square the truth mask is grown by")
    ap.add_argument("--ssim", action="store_true", help="eraser: also the SSIM of every erased page against the clean one")
    ap.add_argument("--seg-model", default="XceptionTextSegment", choices=["XceptionTextSegment", "TextSegament"])
    ap.add_argument("--fill-model", default="ImageFill", choices=["ImageFill", "ImageFillOrigin", "ImageFillOriginV2"])
    ap.add_argument("--seg-checkpoint", default=None)
    ap.add_argument("--fill-checkpoint", default=None)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--halo", type=int, default=64)
    ap.add_argument("--dilate", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--tile-batch", type=int, default=8)
    ap.add_argument("--min-area", type=int, default=0)
    ap.add_argument("--connectivity", type=int, default=8, choices=[4, 8])
    ap.add_argument("--hull", action="store_true")
    ap.add_argument("--seg-long-side", type=int, default=None)
    ap.add_argument("--pack", action="store_true")
    ap.add_argument("--flat", type=int, default=None, metavar="T")
    ap.add_argument("--flat-ring", type=int, default=3, metavar="N")
    ap.add_argument("--smooth", type=int, default=None, metavar="T")
    ap.add_argument("--smooth-ring", type=int, default=3, metavar="N")
    ap.add_argument("--smooth-sweeps", type=int, default=8, metavar="N")
    ap.add_argument("--tone", type=int, default=None, metavar="T")
    ap.add_argument("--tone-ring", type=int, default=8, metavar="N")
    ap.add_argument("--tone-period", type=int, default=12, metavar="N")
    ap.add_argument("--group", type=int, default=None, metavar="G")
    ap.add_argument("--seed", type=float, default=None, metavar="P", help="eraser: keep a text region only if some pixel of it has a probability above P")
    ap.add_argument("--min-seeds", type=int, default=1, metavar="N")
    ap.add_argument("--filler", default="net", choices=["net", "harmonic", "patch"])
    ap.add_argument("--sweeps", type=int, default=8, metavar="N")
    ap.add_argument("--patch", type=int, default=7, metavar="N")
    ap.add_argument("--levels", type=int, default=4, metavar="N")
    ap.add_argument("--iters", type=int, default=4, metavar="N")
    ap.add_argument("--fill-seed", type=int, default=0, metavar="S")
    ap.add_argument("--blend", action="store_true", help="eraser: seamless composition of the filler's output; the line gains without_blend")
    ap.add_argument("--blend-sweeps", type=int, default=8, metavar="N")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="N seeded synthetic images instead of a folder")
    ap.add_argument("--model", default=None, help="default: XceptionTextSegment / ImageFill")
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--thresholds", type=int, default=19, help="segmentation: evenly spaced probabilities swept (1..32)")
    args = ap.parse_args(argv)
    if args.task == "eraser":
        if (args.synthetic > 0) == (args.raw_folder is not None and args.clean_folder is not None):
            ap.error("give either --raw-folder and --clean-folder or --synthetic N")
        return eraser_main(args)
    if (args.synthetic > 0) == (args.img_folder is not None):
        ap.error("give either --img-folder or --synthetic N")
    import text_segmentation_image_inpainting_amd as T
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    name = args.model or ("XceptionTextSegment" if args.task == "segmentation" else "ImageFill")
    net = getattr(T, name)()
    if args.checkpoint:
        net.load_state_dict(torch.load(args.checkpoint, map_location="cpu"))     # the tolerant loader: reports what does not fit
    net = net.to(dev)
    batches = (synthetic_batches(args.task, args.synthetic, args.batch, args.size) if args.synthetic
               else folder_batches(args.task, args.img_folder, args.batch, args.size))
    if args.task == "segmentation":
        res = T.evaluate_segmentation(net, batches, T.SegmentationMetrics(args.thresholds))
        res["suggested_eraser_threshold"] = res["best_threshold"]
    else:
        res = T.evaluate_inpainting(net, batches)
    line = {"task": args.task, "model": name, "checkpoint": args.checkpoint, "size": args.size, **res}
    print(json.dumps(line))
    return line


if __name__ == "__main__":
    main()
