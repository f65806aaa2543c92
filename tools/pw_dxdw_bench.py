"""K3x A/B per layer shape: tsii_pw_bwd_dx + tsii_pw_bwd_dw against tsii_pw_bwd_dxdw through the C ABI.

    python tools/pw_dxdw_bench.py

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
for (m, n, k, split) in ((2097152, 384, 64, 64), (2097152, 256, 64, 0), (524288, 384, 64, 0)):
    dy = torch.randn(m, n, device=dev); x = torch.randn(m, k, device=dev); w = torch.randn(n, k, device=dev) * 0.05
    inv = torch.rand(m, device=dev); r0 = (torch.rand(m, device=dev) > 0.3).float() if split else None
    dx = torch.empty(m, k, device=dev); dw = torch.empty(n, k, device=dev)
    dx2 = torch.empty(m, k, device=dev); dw2 = torch.empty(n, k, device=dev)
    wt = torch.empty(L.tsii_pw_ws_bytes(n, k) // 4 + 4, device=dev)
    nb = L.tsii_pw_bwd_dw_ws_bytes(m, n, k); ws = torch.empty(nb // 4 + 4, device=dev)
    nb2 = L.tsii_pw_bwd_dxdw_ws_bytes(m, n, k); ws2 = torch.empty(nb2 // 4 + 4, device=dev)
    f_dx = lambda: call("tsii_pw_bwd_dx", ptr(dy), m, n, ptr(w), k, ptr(inv), ptr(r0), split, None, ptr(dx), ptr(wt), st)
    f_dw = lambda: call("tsii_pw_bwd_dw", ptr(dy), ptr(x), m, n, k, ptr(inv), None, ptr(r0), split, None, ptr(dw), None, ptr(ws), nb, st)
    f_xw = lambda: call("tsii_pw_bwd_dxdw", ptr(dy), ptr(x), m, n, ptr(w), k, ptr(inv), None, ptr(r0), split, None, ptr(dx2), ptr(dw2), None, ptr(ws2), nb2, st)
    t1, t2, t3 = timeit(f_dx), timeit(f_dw), timeit(f_xw)
    e1 = float((dx - dx2).abs().max() / dx.abs().max()); e2 = float((dw - dw2).abs().max() / dw.abs().max())
    print(f"shape ({m},{n},{k}) split {split}: dx {t1:.3f} ms + dw {t2:.3f} ms = {t1+t2:.3f} | fused {t3:.3f} ms | rel diff dx {e1:.1e} dw {e2:.1e}", flush=True)
    del dy, x, dx, dx2, ws, ws2
