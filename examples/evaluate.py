#!/usr/bin/env python3
"""Validate a checkpoint on the device: precision / recall / F1 / IoU over a threshold sweep for a segmentation net, L1 / PSNR /
SSIM for an inpainting net.  The metrics are accumulated by the kernels of ``csrc/metrics.hip``; the host reads one small result.
Needs an MI355X (the models have no CPU path).  Prints ONE JSON line.

    python examples/evaluate.py --task segmentation --img-folder train/raw [--checkpoint seg.pt] [--thresholds 19]
    python examples/evaluate.py --task inpainting --img-folder clean_pages [--checkpoint fill.pt]
    python examples/evaluate.py --task segmentation --synthetic 8          # seeded synthetic batches, random-init weights

Folders are what ``TextSegmentationData`` / ``ImageInpaintingData`` take.  For segmentation the line carries the sweep and
``suggested_eraser_threshold``: the probability with the best F1, to be passed as ``TextEraser(threshold=...)``.
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--task", required=True, choices=["segmentation", "inpainting"])
    ap.add_argument("--img-folder", default=None)
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="N seeded synthetic images instead of a folder")
    ap.add_argument("--model", default=None, help="default: XceptionTextSegment / ImageFill")
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--thresholds", type=int, default=19, help="segmentation: evenly spaced probabilities swept (1..32)")
    args = ap.parse_args(argv)
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
