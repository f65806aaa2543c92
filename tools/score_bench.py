#!/usr/bin/env python3
"""HIP-event times of the two page-score kernels (csrc/score.hip) on one page of 1170 x 1654 pixels, the size tools/erase_bench.py times
the page pipeline at:

    tsii_pair_text_mask   raw, clean -> truth       thr 102, k 10 (the reference's pair mask)
    tsii_page_scores      out, clean, mask, truth, labels -> page sums and one row per text region

The pair is the seeded one of ``examples/evaluate.py --task eraser --synthetic`` (a manga-like page, and the page with blocks of dark
strokes drawn over it); `out` is the clean page with the strokes' pixels a few grey levels off (so that every sum is exercised), the mask
and the labels come from ``pair_text_mask`` and ``text_regions`` themselves.  Per entry: 3 warm-up calls, then 10 timed samples of
``--inner`` calls between one event pair, median (min - max) per call.  A call is one to three launches of a few microseconds, less than
the host takes to enqueue it: ``ms`` is taken with two large matrix products enqueued in front of the first event, so that the calls
queue up behind them and then run back to back -- the device's time per call, the gaps between launches included; ``host_paced_ms`` is
the same without them, the rate at which Python enqueues.  ``bytes`` are the algorithmic ones -- every input plane read once, every output
written once, the halo re-reads of the pair mask not counted -- and ``tb_per_s`` what they make over ``ms``.  A page's planes are
6 - 25 MB and stay in the 256 MB Infinity Cache between calls: these are warm-cache times, which is how the kernels run behind
TextEraser, whose compose pass has just written the page.  Prints ONE JSON line.  Needs an MI355X.

    python tools/score_bench.py [--out profiles/score_bench_1170x1654.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

WARMUP, SAMPLES = 3, 10


def timed(fn, inner, blocker=None):
    """per-call ms of ``fn``: (median, min, max) over SAMPLES event pairs around ``inner`` calls each.  With ``blocker`` (work of several
    milliseconds enqueued in front of the first event) the calls queue up behind it and then run back to back: the device's time per
    call, launch gaps included; without it the host's enqueue rate paces them."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(SAMPLES):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if blocker is not None:
            blocker()
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return statistics.median(ms), min(ms), max(ms)


def entry(name, nbytes, fn, inner, blocker, **extra):
    ms, paced = timed(fn, inner, blocker), timed(fn, inner)
    return dict(name=name, bytes=int(nbytes), ms=round(ms[0], 5), ms_min=round(ms[1], 5), ms_max=round(ms[2], 5),
                tb_per_s=round(nbytes / (ms[0] * 1e-3) / 1e12, 3), host_paced_ms=round(paced[0], 5), **extra)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, nargs=2, default=(1170, 1654), metavar=("H", "W"))
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/score_bench.py measures on an MI355X: no GPU found")
    import text_segmentation_image_inpainting_amd as T
    from examples.evaluate import synthetic_pairs
    from text_segmentation_image_inpainting_amd import score
    dev = torch.device("cuda:0")
    h, w = args.size
    raw_h, clean_h = next(synthetic_pairs(1, h, w))
    ink = (raw_h != clean_h).any(axis=-1)
    out_h = clean_h.copy()
    out_h[ink] = np.clip(clean_h[ink].astype(np.int16) + (9, -4, 2), 0, 255).astype(np.uint8)
    raw, clean, out = (torch.from_numpy(a).to(dev) for a in (raw_h, clean_h, out_h))
    truth = score._pair_text_mask(raw, clean, 102, 10)
    regions = T.text_regions(truth, max_regions=4096)
    labels, table = regions.labels, score._table_on(regions.table, dev)
    n = h * w
    big = torch.randn(8192, 8192, device=dev)

    def blocker():                                       # about 1.1 TFLOP of fp32 each: several milliseconds, while the host enqueues
        torch.mm(big, big)
        torch.mm(big, big)
    rows = int(table.shape[0])
    entries = [entry("tsii_pair_text_mask", 7 * n, lambda: score._pair_text_mask(raw, clean, 102, 10), args.inner, blocker, launches=1),
               entry("tsii_page_scores", 12 * n + 32 * rows, lambda: score._page_scores(out, clean, truth, truth, labels, table), args.inner,
                     blocker, launches=3, rows=rows),
               entry("tsii_page_scores (no labels)", 8 * n, lambda: score._page_scores(out, clean, truth, truth), args.inner, blocker,
                     launches=2, rows=0)]
    got = T.score_page(out, clean, truth, truth, labels, table)
    line = {"tool": "score_bench", "page": [h, w], "inner": args.inner, "samples": SAMPLES, "warmup": WARMUP,
            "text_fraction": round(float((truth != 0).float().mean()), 4), "regions": int(table.shape[0]),
            "page_sums": [int(v) for v in got["page"]],
            "entries": entries}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
    return line


if __name__ == "__main__":
    main()
