#!/usr/bin/env python3
"""HIP-event times of the three validation-metric kernels (csrc/metrics.hip) at the sizes a validation loop runs them:

    tsii_ssim, tsii_inpaint_errors   32 x 512 x 512 x 3      (one ImageFill batch)
    tsii_seg_confusion               64 x 512 x 512, K = 1 and K = 19 thresholds

beside a restatement in torch on the same device made of element-wise ops, reductions and shifted slices only (no convolution
library call) -- what a user would write without the kernels.  Per entry: 3 warm-up calls, then 10 timed samples of ``--inner``
back-to-back calls between one event pair (a single 50 us launch is too short for an event pair), median (min - max) per call;
algorithmic bytes (every input read once, the ring re-reads of the SSIM tiles not counted) and the TB/s they make.  The calls
alternate between two sets of inputs, so that a call never finds its 100 - 200 MB of inputs left in the 256 MB Infinity Cache
by the call before.  The ImageFill forward (bs 32, 512 x 512, no_grad, eval) is timed in the same run for SSIM's share of it.
Prints ONE JSON line.  Needs an MI355X.

    python tools/metrics_bench.py [--out profiles/metrics_bench_512.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

WARMUP, SAMPLES = 3, 10


def timed(fn_sets, inner):
    """fn_sets: callables doing the same work on different inputs, called in turn -> per-call ms: (median, min, max)"""
    k = 0
    for _ in range(WARMUP):
        for f in fn_sets:
            f()
    torch.cuda.synchronize()
    ms = []
    for _ in range(SAMPLES):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn_sets[k % len(fn_sets)]()
            k += 1
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return statistics.median(ms), min(ms), max(ms)


def entry(name, shape, nbytes, kernel, torch_fn, inner, torch_inner):
    km = timed(kernel, inner)
    tm = timed(torch_fn, torch_inner)
    return {"name": name, "shape": shape, "bytes": nbytes, "kernel_ms": round(km[0], 5), "kernel_ms_min": round(km[1], 5),
            "kernel_ms_max": round(km[2], 5), "kernel_tb_per_s": round(nbytes / (km[0] * 1e-3) / 1e12, 3),
            "torch_ms": round(tm[0], 4), "torch_ms_min": round(tm[1], 4), "torch_ms_max": round(tm[2], 4),
            "torch_tb_per_s": round(nbytes / (tm[0] * 1e-3) / 1e12, 4), "speedup": round(tm[0] / km[0], 2)}


# ---- torch restatements ------------------------------------------------------------------------------------------------------------
def torch_confusion(logits, target, thr):
    text = target > 0.5
    exceeded = torch.zeros_like(logits, dtype=torch.int32)
    for t in thr:
        exceeded += logits > t
    bins = []
    for b in range(len(thr) + 1):
        at = exceeded == b
        txt = (at & text).sum(dim=(1, 2))
        bins.append(torch.stack([at.sum(dim=(1, 2)) - txt, txt], dim=1))
    return torch.stack(bins, dim=2)


def torch_errors(out, clean, plane):
    d = out.clamp(0.0, 1.0) - clean
    hole = (~(plane > 0.5)).unsqueeze(-1)
    ad, d2 = d.abs().double(), d.double() ** 2
    cnt = hole.sum(dim=(1, 2, 3)).double() * out.shape[3]
    return torch.stack([cnt, (ad * hole).sum(dim=(1, 2, 3)), (d2 * hole).sum(dim=(1, 2, 3)), (ad * ~hole).sum(dim=(1, 2, 3)),
                        (d2 * ~hole).sum(dim=(1, 2, 3))], dim=1)


def torch_ssim(a, b, g, data_range=1.0):
    h, w = a.shape[1], a.shape[2]
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2

    def blur(f):
        hz = g[0] * f[:, :, 0:w - 10]
        for j in range(1, 11):
            hz = hz + g[j] * f[:, :, j:j + w - 10]
        v = g[0] * hz[:, 0:h - 10]
        for i in range(1, 11):
            v = v + g[i] * hz[:, i:i + h - 10]
        return v
    mu_a, mu_b = blur(a), blur(b)
    var_a, var_b, cov = blur(a * a) - mu_a * mu_a, blur(b * b) - mu_b * mu_b, blur(a * b) - mu_a * mu_b
    s = ((2 * mu_a * mu_b + c1) * (2 * cov + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (var_a + var_b + c2))
    return s.double().mean(dim=(1, 2, 3))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32, help="images for SSIM / errors; the confusion kernel gets twice as many")
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench needs an MI355X: a CPU run cannot give a time")
    import math
    import text_segmentation_image_inpainting_amd as T
    from text_segmentation_image_inpainting_amd import metrics as M
    from text_segmentation_image_inpainting_amd.pipeline import logit_of
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    n, s = args.batch, args.size
    res = {"tool": "metrics_bench", "device": torch.cuda.get_device_name(0), "size": s, "warmup": WARMUP, "samples": SAMPLES,
           "inner": args.inner, "entries": []}
    # inpainting: two sets of (out, clean, plane)
    sets = []
    for _ in range(2):
        clean = torch.rand(n, s, s, 3, device=dev)
        out = clean + 0.1 * torch.randn(n, s, s, 3, device=dev)
        plane = (torch.rand(n, s, s, device=dev) < 0.8).float()
        sets.append((out, clean, plane))
    g = [math.exp(-((i - 5) ** 2) / (2 * 1.5 ** 2)) for i in range(11)]
    g = [v / sum(g) for v in g]
    ks, ts = M._ssim(*sets[0][:2]), torch_ssim(*sets[0][:2], g)
    res["ssim_kernel_vs_torch_max_abs"] = float((ks - ts).abs().max())
    res["entries"].append(entry("tsii_ssim", [n, s, s, 3], 2 * n * s * s * 3 * 4, [lambda q=q: M._ssim(q[0], q[1]) for q in sets],
                                [lambda q=q: torch_ssim(q[0], q[1], g) for q in sets], args.inner, 2))
    ke, te = M._inpaint_errors(*sets[0], True), torch_errors(*sets[0])
    res["errors_kernel_vs_torch_max_rel"] = float(((ke - te).abs() / te.abs().clamp_min(1e-30)).max())
    res["entries"].append(entry("tsii_inpaint_errors (plane mask, clamp)", [n, s, s, 3], n * s * s * (2 * 3 + 1) * 4,
                                [lambda q=q: M._inpaint_errors(q[0], q[1], q[2], True) for q in sets],
                                [lambda q=q: torch_errors(*q) for q in sets], args.inner, 2))
    del sets
    # segmentation: two sets of (logits, target)
    segs = [(3 * torch.randn(2 * n, s, s, device=dev), (torch.rand(2 * n, s, s, device=dev) < 0.3).float()) for _ in range(2)]
    for k in (1, 19):
        thr = [logit_of((i + 1) / (k + 1)) for i in range(k)]
        assert torch.equal(M._seg_confusion(*segs[0], thr).long(), torch_confusion(*segs[0], thr))
        res["entries"].append(entry("tsii_seg_confusion K=%d" % k, [2 * n, s, s], 2 * 2 * n * s * s * 4,
                                    [lambda q=q: M._seg_confusion(q[0], q[1], thr) for q in segs],
                                    [lambda q=q: torch_confusion(q[0], q[1], thr) for q in segs], args.inner, 2))
    del segs
    if not args.no_forward:
        net = T.ImageFill().to(dev).eval()
        c, m, _ = (torch.rand(n, 3, s, s, device=dev).contiguous(memory_format=torch.channels_last) for _ in range(3))
        m = (m[:, :1] < 0.8).float().expand(-1, 3, -1, -1)
        with torch.no_grad():
            fwd = timed([lambda: net((c * m, m))], 2)
        res["imagefill_forward_ms"] = round(fwd[0], 3)
        res["ssim_share_of_imagefill_forward"] = round(res["entries"][0]["kernel_ms"] / fwd[0], 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
