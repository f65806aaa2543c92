"""K4s A/B: tsii_act_bwd + tsii_dense_bwd_dw against tsii_stem_bwd through the C ABI, at the headline workload's stem (n = 32,
512^2 image: x2 259 x 259 x 12, 256 x 256 x 64 output) and at n = 8.

    python tools/stem_bwd_bench.py            # one child process per shape, each under its own time limit; stops at the first failure
    python tools/stem_bwd_bench.py --n 32     # one shape in this process

Each figure is the mean of 10 back-to-back calls between two stream events after 3 warm-up calls, on random operands, whole entry
points (partial-slab reductions included).  Back-to-back repeats of one call read higher than the same launch inside a training step;
compare the columns of one run with each other.  TB/s: gy and y (2 x m x 64 floats) over the fused call's time; the floor of the fused
call is those two reads plus x2 once."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 120


def one(n):
    import torch
    sys.path.insert(0, ROOT)
    from text_segmentation_image_inpainting_amd import _lib
    from text_segmentation_image_inpainting_amd._lib import call, ptr
    L = _lib.lib(); st = _lib.stream(); dev = "cuda"

    def timeit(fn, reps=10):
        for _ in range(3): fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps): fn()
        b.record(); torch.cuda.synchronize()
        return a.elapsed_time(b) / reps
    ho = wo = 256; h2 = w2 = 259; c4, cout, ka, slope = 12, 64, 4, 0.3
    m = n * ho * wo
    gy = torch.randn(m, cout, device=dev); y = torch.randn(m, cout, device=dev); dy = torch.empty_like(gy)
    x2 = torch.randn(n, h2, w2, c4, device=dev)
    keep = (torch.rand(m, device=dev) > 0.1).float(); inv = keep / torch.randint(1, 9, (m,), device=dev).float()
    dw1 = torch.empty(cout, c4, ka, ka, device=dev); db1 = torch.empty(cout, device=dev)
    dw2 = torch.empty(cout, c4, ka, ka, device=dev); db2 = torch.empty(cout, device=dev)
    nb1 = L.tsii_dense_bwd_dw_ws_bytes(n, ho, wo, c4, cout, ka, ka); ws1 = torch.empty(nb1 // 4 + 4, device=dev)
    assert L.tsii_stem_bwd_ok(ptr(gy), ptr(y), ptr(x2), n, h2, w2, c4, cout, ka, ka, 1, ho, wo) == 1
    nb2 = L.tsii_stem_bwd_ws_bytes(n, ho, wo); ws2 = torch.empty(nb2 // 4 + 4, device=dev)
    f_act = lambda: call("tsii_act_bwd", ptr(gy), ptr(y), m * cout, 2, slope, ptr(dy), st)
    f_dw = lambda: call("tsii_dense_bwd_dw", ptr(dy), ptr(inv), ptr(keep), ptr(x2), None, None, 0, None, n, h2, w2, c4, cout,
                        ka, ka, 1, 1, 0, 0, 1, 1, ho, wo, ptr(dw1), ptr(db1), ptr(ws1), nb1, st)
    f_new = lambda: call("tsii_stem_bwd", ptr(gy), ptr(y), slope, ptr(inv), ptr(keep), ptr(x2), n, h2, w2, c4, cout, ka, ka, 1, ho, wo,
                         ptr(dw2), ptr(db2), ptr(ws2), nb2, st)
    f_new_a = lambda: call("tsii_stem_bwd", ptr(dy), None, slope, ptr(inv), ptr(keep), ptr(x2), n, h2, w2, c4, cout, ka, ka, 1, ho, wo,
                           ptr(dw2), ptr(db2), ptr(ws2), nb2, st)
    t_act, t_dw, t_a, t_new = timeit(f_act), timeit(f_dw), timeit(f_new_a), timeit(f_new)
    e_w = float((dw1 - dw2).abs().max() / dw1.abs().max()); e_b = float((db1 - db2).abs().max() / db1.abs().max())
    gb = 2.0 * m * cout * 4 / 1e9
    floor_gb = gb + x2.numel() * 4 / 1e9
    print(f"n {n} (m {m}): act_bwd {t_act:.3f} ms + dense_bwd_dw {t_dw:.3f} ms = {t_act + t_dw:.3f} | stem_bwd without y {t_a:.3f} ms | "
          f"stem_bwd {t_new:.3f} ms = {gb / t_new:.2f} TB/s of gradient + output read (floor {floor_gb:.2f} GB) | "
          f"rel diff dwk {e_w:.1e} db {e_b:.1e}", flush=True)


if __name__ == "__main__":
    if "--n" in sys.argv:
        one(int(sys.argv[sys.argv.index("--n") + 1]))
    else:
        for n in (32, 8):
            rc = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--n", str(n)]).returncode
            if rc != 0:
                sys.exit(f"n = {n}: exit status {rc}; nothing further is started")
