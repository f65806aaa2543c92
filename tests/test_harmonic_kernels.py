"""Harmonic fill (csrc/harmonic.hip, include/tsii_hip.h "K14: harmonic fill") through the C ABI on the emulator (CPU suite) and, with
-m gpu, on the chip: the holes of an image take the smooth continuation of the valid pixels around them, in one coarse-to-fine pass.

The semantics, restated in numpy float64 (``harmonic_ref``) in another structure than the kernels' patches: the pyramid as padded
reshape-sums over 2 x 2 cells, the push as ``np.repeat``, a Jacobi sweep as four whole-array shifts of a zero-padded level.

The bound is derived, not tuned.  With ``L`` levels above the image every value is built by ``D = L + L (1 + sweeps)`` sequential
averaging steps (L pulls, then per level one push and ``sweeps`` sweeps); a step is at most 3 additions and a division = 4 fp32
roundings of values no larger than ``max |valid x|``, and a later step cannot amplify an earlier error because it is a convex
combination.  So ``|device - float64| <= D * 4 * 2^-24 * max |valid x|`` (2.1e-5 for 512 x 512, 8 sweeps, inputs in [0, 1]).

Every output carries a canary tail; the workspace is handed over full of canary bytes and is exactly ``tsii_harmonic_fill_ws_bytes``
long in front of its own canary tail.
"""
import functools

import numpy as np
import pytest
import torch

from tests.backends import BACKENDS, both_backends
from tests.test_pipeline_kernels import Buf, up
from text_segmentation_image_inpainting_amd import _lib

SHAPES = [(1, 1, 1), (1, 1, 7), (2, 5, 3), (1, 33, 65), (3, 64, 64), (1, 65, 64), (2, 150, 217)]
SWEEPS16 = [(1, 33, 65), (2, 150, 217)]
PATTERNS = ["blocks", "big", "checker", "glyphs", "none", "all", "single"]
IDS = dict(ids=lambda s: "x".join(str(v) for v in s))


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def levels_above(h, w):
    n = 0
    while h > 1 or w > 1:
        h, w, n = (h + 1) // 2, (w + 1) // 2, n + 1
    return n


def bound_of(h, w, sweeps, peak):
    lv = levels_above(h, w)
    return (lv + lv * (1 + sweeps)) * 4 * 2.0 ** -24 * peak


def harmonic_ref(x, valid, sweeps):
    """one image: x [h, w, 3] (anything under the holes), valid bool [h, w] -> float64 [h, w, 3]"""
    vs, ms = [np.where(valid[..., None], x.astype(np.float64), 0.0)], [valid.astype(bool)]
    while vs[-1].shape[:2] != (1, 1):
        v, m = vs[-1], ms[-1]
        h, w = m.shape
        hc, wc = (h + 1) // 2, (w + 1) // 2
        vp, mp = np.zeros((2 * hc, 2 * wc, 3)), np.zeros((2 * hc, 2 * wc))
        vp[:h, :w], mp[:h, :w] = np.where(m[..., None], v, 0.0), m
        total, count = vp.reshape(hc, 2, wc, 2, 3).sum(axis=(1, 3)), mp.reshape(hc, 2, wc, 2).sum(axis=(1, 3))
        ms.append(count > 0)
        vs.append(total / np.maximum(count, 1)[..., None])
    u = np.where(ms[-1][..., None], vs[-1], 0.0)
    for lv in range(len(vs) - 2, -1, -1):
        m = ms[lv]
        h, w = m.shape
        u = np.where(m[..., None], vs[lv], np.repeat(np.repeat(u, 2, axis=0), 2, axis=1)[:h, :w])
        present = np.pad(np.ones((h, w)), 1)
        count = present[:-2, 1:-1] + present[2:, 1:-1] + present[1:-1, :-2] + present[1:-1, 2:]
        for _ in range(sweeps):
            p = np.pad(u, ((1, 1), (1, 1), (0, 0)))
            total = p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:]
            u = np.where(m[..., None], u, total / count[..., None])
    return u


# ---- holes -----------------------------------------------------------------------------------------------------------------------
def holes(name, h, w, seed=0):
    """bool [h, w], True = hole"""
    t = np.zeros((h, w), bool)
    if name == "blocks":        # across the patch lines x = 63 / 64 and y = 31 / 32, against all four edges and in the corners
        rects = [(0, 0, 3, 5), (h - 3, w - 6, h, w), (0, w - 4, 2, w), (h - 2, 0, h, 3), (28, 58, 37, 70), (29, 120, 35, 131), (60, 61, 68, 66),
                 (h // 2 - 2, 0, h // 2 + 2, 4), (h // 2 - 2, w - 3, h // 2 + 2, w), (0, w // 2, 3, w // 2 + 9), (h - 2, w // 2, h, w // 2 + 9),
                 (90, 30, 99, 41), (92, 44, 97, 50), (100, 150, 120, 190)]
        for y0, x0, y1, x1 in rects:
            if 0 <= y0 < y1 <= h and 0 <= x0 < x1 <= w:
                t[y0:y1, x0:x1] = True
        if h * w <= 7:
            t[0, w // 2] = True
    elif name == "big":         # the 40 x 120 block, clipped to the smaller images
        if h >= 100 and w >= 180:
            t[55:95, 50:170] = True
        else:
            t[h // 3:h - h // 4, w // 4:w - w // 4] = True
    elif name == "checker":
        t[(np.add.outer(np.arange(h), np.arange(w)) % 2) == 1] = True
    elif name == "glyphs":
        rng = np.random.default_rng(100 + seed + 7 * h + w)
        for _ in range(max(1, h * w // 540)):
            gh, gw = int(rng.integers(2, 9)), int(rng.integers(2, 13))
            y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
            t[y:y + gh, x:x + gw] = True
    elif name == "all":
        t[:] = True
    elif name == "single":      # everything a hole but one pixel
        t[:] = True
        t[(2 * h) // 3, w // 3] = False
    else:
        assert name == "none"
    return t


@functools.lru_cache(maxsize=None)
def case(name, n, h, w, sweeps):
    """(x fp32 [n, h, w, 3] in [0, 1), hole planes bool [n, h, w], float64 reference): computed once; callers do not modify it"""
    rng = np.random.default_rng(1000 + 31 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    x = np.stack([(0.25 + 0.5 * rng.random((h, w, 3)) * (k % 2) + 0.2 * np.sin(yy / 7.0 + k)[..., None] + 0.2 * np.cos(xx / 9.0)[..., None]
                   + 0.05 * rng.random((h, w, 3))) for k in range(n)]).astype(np.float32)
    x = np.clip(x, 0.0, 1.0)
    hole = np.stack([holes(name, h, w, seed=k) for k in range(n)])
    ref = np.stack([harmonic_ref(x[k], ~hole[k], sweeps) for k in range(n)])
    return x, hole, ref


# ---- the kernels -----------------------------------------------------------------------------------------------------------------
def run(dev, x, hole, sweeps, ws=None, **bad):
    """one call -> (out [n, h, w, 3] fp32, the workspace Buf); the canary tails of out and ws are checked"""
    n, h, w = hole.shape
    lib = _lib.lib()
    nbytes = lib.tsii_harmonic_fill_ws_bytes(n, h, w)
    assert nbytes > 0 and nbytes % 4 == 0 and (h * w < 4096 or nbytes <= 0.4 * x.nbytes), "roughly a third of the input again"
    xd, md = up(dev, x), up(dev, (~hole).astype(np.float32))
    out = Buf(dev, x.size, torch.float32)
    ws = Buf(dev, nbytes // 4, torch.float32) if ws is None else ws
    a = dict(x=_lib.ptr(xd), mask=_lib.ptr(md), n=n, h=h, w=w, sweeps=sweeps, out=out.ptr, ws=ws.ptr)
    a.update(bad)
    _lib.call("tsii_harmonic_fill", a["x"], a["mask"], a["n"], a["h"], a["w"], a["sweeps"], a["out"], a["ws"], _lib.stream())
    got = out.get().reshape(n, h, w, 3)
    ws.get()
    assert np.array_equal(xd.cpu().numpy(), x, equal_nan=True), "x is read only"
    return got, ws


def check(got, x, hole, ref, sweeps, name):
    n, h, w = hole.shape
    valid = ~hole
    peak = float(np.abs(x[valid]).max()) if valid.any() else 0.0
    bound = bound_of(h, w, sweeps, peak)
    assert np.isfinite(got).all()
    assert np.array_equal(got[valid].view(np.uint32), x[valid].view(np.uint32)), "valid pixels come back bit for bit"
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{name} {n}x{h}x{w} sweeps {sweeps}: max |device - float64| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (name, err, bound)
    for k in range(n):
        if not valid[k].any():
            assert not got[k].any(), "an image without a valid pixel comes back as zeros"
            continue
        lo, hi = x[k][valid[k]].min(axis=0), x[k][valid[k]].max(axis=0)
        assert bool((got[k] >= lo - bound).all()) and bool((got[k] <= hi + bound).all()), "a convex combination of the valid inputs"
    if name == "none":
        assert np.array_equal(got.view(np.uint32), x.view(np.uint32))
    if name == "all":
        assert not got.any()
    if name == "single":
        for k in range(n):
            colour = x[k][valid[k]].reshape(3)
            assert float(np.abs(got[k] - colour).max()) <= bound, "one valid pixel: its colour everywhere"


def run_shape(backend, shape, sweeps):
    n, h, w = shape
    with BACKENDS[backend]() as dev:
        for name in PATTERNS:
            x, hole, ref = case(name, n, h, w, sweeps)
            got, _ = run(dev, x, hole, sweeps)
            check(got, x, hole, ref, sweeps, name)
            # NaN under every hole: never read, so the same bits
            poisoned = x.copy()
            poisoned[hole] = np.nan
            again, _ = run(dev, poisoned, hole, sweeps)
            assert np.isfinite(again).all() and np.array_equal(again.view(np.uint32), got.view(np.uint32)), name


@both_backends
@pytest.mark.parametrize("sweeps", [0, 1, 8])
@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_against_the_restatement(backend, shape, sweeps):
    run_shape(backend, shape, sweeps)


@both_backends
@pytest.mark.parametrize("shape", SWEEPS16, **IDS)
def test_sixteen_sweeps(backend, shape):
    """the widest apron: 64 x 96 staged pixels per block"""
    run_shape(backend, shape, 16)


@pytest.mark.gpu
@pytest.mark.parametrize("sweeps", [0, 1, 8])
def test_pipeline_tile(sweeps):
    """CHIP ONLY: two tiles of the pipeline's 512 x 512 (three fine levels, the 16-byte paths)"""
    run_shape("gpu", (2, 512, 512), sweeps)


@both_backends
def test_two_runs_and_a_used_workspace(backend):
    """the same call twice, the second time on the workspace another shape left behind: identical bits"""
    x, hole, ref = case("blocks", 2, 150, 217, 8)
    xs, holes_s, _ = case("glyphs", 1, 65, 64, 8)
    with BACKENDS[backend]() as dev:
        first, ws = run(dev, x, hole, 8)
        run(dev, xs, holes_s, 8, ws=ws)                   # a smaller problem in the same (larger) workspace
        second, _ = run(dev, x, hole, 8, ws=ws)
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32))


@both_backends
@pytest.mark.parametrize("shape", [(3, 64, 64), (2, 150, 217)], **IDS)
def test_batch_images_equal_the_image_alone(backend, shape):
    n, h, w = shape
    names = ["glyphs", "blocks", "checker"][:n]
    parts = [case(name, n, h, w, 8) for name in names]
    x = np.stack([parts[k][0][k] for k in range(n)])
    hole = np.stack([parts[k][1][k] for k in range(n)])
    with BACKENDS[backend]() as dev:
        together, _ = run(dev, x, hole, 8)
        alone = [run(dev, x[k:k + 1], hole[k:k + 1], 8)[0][0] for k in range(n)]
    for k in range(n):
        assert np.array_equal(together[k].view(np.uint32), alone[k].view(np.uint32)), k
        assert float(np.abs(together[k] - parts[k][2][k]).max()) <= bound_of(h, w, 8, 1.0)


@both_backends
def test_ramp(backend):
    """the test that says it inpaints: a 150 x 217 ramp page with a 40 x 120 interior hole, 8 sweeps, comes back within one grey level
    of the ramp (the exact solution of the Laplace system there is the ramp itself; the restatement is 0.00392 from it with this hole,
    0.0030 after 16 sweeps)"""
    h, w = 150, 217
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = 0.2 + 0.5 * xx / w + 0.25 * yy / h
    x = np.stack([ramp, 0.9 - 0.6 * ramp, 0.1 + 0.8 * ramp], axis=-1).astype(np.float32)[None]
    hole = np.zeros((1, h, w), bool)
    hole[0, 55:95, 50:170] = True
    ref = harmonic_ref(x[0], ~hole[0], 8)[None]
    dev_of_ramp = float(np.abs(ref - x.astype(np.float64)).max())
    print(f"restatement - ramp: {dev_of_ramp:.4f}")
    assert dev_of_ramp <= 1.0 / 255.0
    poisoned = x.copy()
    poisoned[hole] = np.nan
    with BACKENDS[backend]() as dev:
        got, _ = run(dev, poisoned, hole, 8)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"device - restatement: {err:.3e}, bound {bound_of(h, w, 8, float(x.max())):.3e}")
    assert err <= bound_of(h, w, 8, float(x.max()))


@both_backends
def test_refusals(backend):
    x, hole, _ = case("blocks", 2, 5, 3, 8)
    lib = _lib.lib
    with BACKENDS[backend]() as dev:
        for n, h, w in ((0, 5, 3), (2, 0, 3), (2, 5, 0), (-1, 5, 3), (1, 26755, 26755), (2 ** 20, 2 ** 10, 1)):
            assert lib().tsii_harmonic_fill_ws_bytes(n, h, w) == 0, (n, h, w)
        assert lib().tsii_harmonic_fill_ws_bytes(1, 26754, 26754) > 0
        xd = up(dev, x)
        outs = []
        for bad in (dict(n=0), dict(h=0), dict(w=0), dict(n=-2), dict(h=26755, w=26755), dict(sweeps=-1), dict(sweeps=17), dict(x=None),
                    dict(mask=None), dict(out=None), dict(ws=None), dict(x=_lib.ptr(xd), out=_lib.ptr(xd))):
            n, h, w = hole.shape
            out, ws = Buf(dev, x.size, torch.float32), Buf(dev, lib().tsii_harmonic_fill_ws_bytes(n, h, w) // 4, torch.float32)
            a = dict(x=_lib.ptr(xd), mask=_lib.ptr(up(dev, (~hole).astype(np.float32))), n=n, h=h, w=w, sweeps=8, out=out.ptr, ws=ws.ptr)
            a.update(bad)
            with pytest.raises(RuntimeError, match=r"tsii_harmonic_fill failed \(-?[1-9]\d*\): harmonic_fill: "):
                _lib.call("tsii_harmonic_fill", a["x"], a["mask"], a["n"], a["h"], a["w"], a["sweeps"], a["out"], a["ws"], _lib.stream())
            outs.append((out.get(), ws.get()))
        x_after = xd.cpu().numpy()
    for out, ws in outs:
        assert bool((out.view(np.uint8) == 0xA5).all()) and bool((ws.view(np.uint8) == 0xA5).all()), "a refused call launches nothing"
    assert np.array_equal(x_after, x)
