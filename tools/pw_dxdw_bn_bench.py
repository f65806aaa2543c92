"""K3xb A/B per layer shape: tsii_bn_bwd_apply + tsii_pw_bwd_dxdw against tsii_pw_bwd_dxdw_bn through the C ABI.

    python tools/pw_dxdw_bn_bench.py

Each figure is the mean of 10 back-to-back calls between two stream events after 3 warm-up calls, on random operands, whole entry
points (weight split, partial-slab reduction included).  Back-to-back repeats of one call on a cold-clock device read higher than
the same launch inside a training step (profiles/*_per_shape.log); compare the columns of one run with each other."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from text_segmentation_image_inpainting_amd import _lib
from text_segmentation_image_inpainting_amd._lib import call, ptr
L = _lib.lib(); st = _lib.stream(); dev = "cuda"
def timeit(fn, n=10):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n
ACT_LEAKY, SLOPE = 2, 0.3
for (m, n, k) in ((2097152, 256, 64), (524288, 256, 64)):
    da = torch.randn(m, n, device=dev); y = torch.randn(m, n, device=dev) * 1.5 + 0.3
    x = torch.randn(m, k, device=dev); w = torch.randn(n, k, device=dev) * 0.05
    inv = torch.rand(m, device=dev) * (torch.rand(m, device=dev) > 0.25)
    coef = torch.stack([torch.randn(n, device=dev) * 0.5, torch.rand(n, device=dev) + 0.5, torch.rand(n, device=dev) + 0.5,
                        torch.randn(n, device=dev) * 0.3, torch.randn(n, device=dev) * 0.05, torch.randn(n, device=dev) * 0.05]).contiguous()
    dy = torch.empty(m, n, device=dev)
    dx = torch.empty(m, k, device=dev); dw = torch.empty(n, k, device=dev)
    dx2 = torch.empty(m, k, device=dev); dw2 = torch.empty(n, k, device=dev)
    nb = L.tsii_pw_bwd_dxdw_ws_bytes(m, n, k); ws = torch.empty(nb // 4 + 4, device=dev)
    nb2 = L.tsii_pw_bwd_dxdw_bn_ws_bytes(m, n, k); ws2 = torch.empty(nb2 // 4 + 4, device=dev)
    f_ap = lambda: call("tsii_bn_bwd_apply", ptr(da), ptr(y), m, n, ptr(coef), ACT_LEAKY, SLOPE, ptr(dy), st)
    f_xw = lambda: call("tsii_pw_bwd_dxdw", ptr(dy), ptr(x), m, n, ptr(w), k, ptr(inv), None, None, 0, None, ptr(dx), ptr(dw), None, ptr(ws), nb, st)
    f_bn = lambda: call("tsii_pw_bwd_dxdw_bn", ptr(da), ptr(y), ptr(coef), ACT_LEAKY, SLOPE, ptr(x), m, n, ptr(w), k, ptr(inv), None, None, 0, None,
                        ptr(dx2), ptr(dw2), None, ptr(ws2), nb2, st)
    t1, t2, t3 = timeit(f_ap), timeit(f_xw), timeit(f_bn)
    same = bool(torch.equal(dx, dx2)) and bool(torch.equal(dw, dw2))
    gbs = 2.0 * m * n * 4 / t3 / 1e6
    print(f"shape ({m},{n},{k}): apply {t1:.3f} ms + dxdw {t2:.3f} ms = {t1+t2:.3f} | fused {t3:.3f} ms ({gbs:.0f} GB/s of da + y) | "
          f"same bits {same}", flush=True)
    del da, y, dy, x, dx, dx2, ws, ws2
