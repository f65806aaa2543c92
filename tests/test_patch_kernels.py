"""Patch fill (csrc/patch.hip, include/tsii_hip.h "K21: patch fill") through the C ABI on the emulator (CPU suite) and, with -m gpu, on the
chip: every hole pixel becomes a copy of a page pixel whose (2r+1)^2 neighbourhood matches, by a coarse-to-fine search of a
nearest-neighbour field (``tsii_patch_fill``).

Everything is an integer, so every comparison is EQUALITY with a restatement of the header's definition in another structure than the
kernels' (which give a lane one hole pixel and let it walk its candidates against a tile of T staged in LDS): ``patch_ref`` works on all
hole pixels of an image at once, one candidate INDEX at a time -- the current source, the 16 propagation candidates, one per search radius
-- with costs from windows gathered out of the whole arrays, the winner as the minimum of ``cost * h * w + sy * w + sx``, the pyramid by
sums over a zero-padded ``[hc, 2, wc, 2]`` view, admissibility as the complement of a max-pool dilation of the hole plane
(``dilate_np``) inside the frame of width r, and the hash in ``np.uint64`` arithmetic masked to 32 bits.

Pages are the quarters of ``tests/test_tone_kernels.py`` (dot lattice, stripes, noise, one colour); ``init`` is random bytes: the kernel
must not depend on a smooth first guess.  Every output carries a canary tail; the workspace is handed over full of canary bytes and is
exactly ``tsii_patch_fill_ws_bytes`` long in front of its own canary tail.
"""
import functools

import numpy as np
import pytest
import torch

from tests.backends import BACKENDS, both_backends
from tests.test_pipeline_kernels import Buf, up
from tests.test_text_eraser import dilate_np
from tests.test_tone_kernels import quarters_page
from text_segmentation_image_inpainting_amd import _lib

SHAPES = [(1, 1, 1), (1, 5, 217), (1, 40, 50), (1, 150, 217), (2, 40, 50)]      # 150 x 217: more than one 32 x 16 block both ways
# (radius, levels, iters, seed): radius 1, 3, 4; levels 1, 3; iters 1, 3; two seeds
PARAMS = [(1, 1, 1, 0), (1, 3, 3, 5), (3, 3, 3, 0), (3, 1, 1, 5), (4, 3, 1, 5), (4, 1, 3, 0)]
KINDS = ["rects", "one", "edge", "full", "none"]
IDS = dict(ids=lambda v: "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v))
M32 = np.uint64(0xFFFFFFFF)
GOLDEN = 0x9E3779B9


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def mix(v):
    v = v & M32
    v = v ^ (v >> np.uint64(16))
    v = (v * np.uint64(0x7FEB352D)) & M32
    v = v ^ (v >> np.uint64(15))
    v = (v * np.uint64(0x846CA68B)) & M32
    return v ^ (v >> np.uint64(16))


def pull_ref(W, H):
    h, w = H.shape
    hc, wc = (h + 1) // 2, (w + 1) // 2
    Wp, on, Hp = np.zeros((2 * hc, 2 * wc, 3), np.int64), np.zeros((2 * hc, 2 * wc), np.int64), np.zeros((2 * hc, 2 * wc), bool)
    Wp[:h, :w], on[:h, :w], Hp[:h, :w] = W, 1, H
    cnt = on.reshape(hc, 2, wc, 2).sum(axis=(1, 3))
    total = Wp.reshape(hc, 2, wc, 2, 3).sum(axis=(1, 3))
    return (total + (cnt // 2)[..., None]) // cnt[..., None], Hp.reshape(hc, 2, wc, 2).any(axis=(1, 3))


def admissible_ref(H, r):
    h, w = H.shape
    frame = np.zeros((h, w), bool)
    frame[r:h - r, r:w - r] = True
    return frame & (dilate_np(H, 2 * r + 1) == 0)


def window_cost(T, W, ys, xs, cy, cx, r):
    h, w = T.shape[:2]
    cost = np.zeros(len(ys), np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ty, tx = ys + dy, xs + dx
            on = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
            t = T[np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)]
            cost += on * np.abs(t - W[cy + dy, cx + dx]).sum(axis=-1)
    return cost


def iterate_ref(W, H, A, fy, fx, r, key):
    """one Jacobi iteration of one image at one level -> the new (fy, fx); -1 = none"""
    h, w = H.shape
    ys, xs = np.nonzero(H)
    if len(ys) == 0:
        return fy, fx
    sourced = H & (fy >= 0)
    T = W.copy()
    T[sourced] = W[fy[sourced], fx[sourced]]
    py, px = fy[ys, xs], fx[ys, xs]
    has = py >= 0
    cands = [(py, px, has)]
    for k in (1, 2, 4, 8):
        for ey, ex in ((0, 1), (0, -1), (1, 0), (-1, 0)):
            qy, qx = ys + k * ey, xs + k * ex
            inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
            cands.append((fy[qy, qx] - k * ey, fx[qy, qx] - k * ex, inside & sourced[qy, qx]))
    cy0, cx0 = np.where(has, py, ys), np.where(has, px, xs)
    hp = mix(mix(np.uint64(key) ^ ys.astype(np.uint64)) ^ xs.astype(np.uint64))
    j, rad = 0, max(h, w)
    while rad >= 1:
        u = mix(hp ^ np.uint64((GOLDEN * (j + 1)) & 0xFFFFFFFF))
        m = np.uint64(2 * rad + 1)
        oy = (((u & np.uint64(0xFFFF)) * m) >> np.uint64(16)).astype(np.int64) - rad
        ox = (((u >> np.uint64(16)) * m) >> np.uint64(16)).astype(np.int64) - rad
        cands.append((cy0 + oy, cx0 + ox, np.ones(len(ys), bool)))
        j, rad = j + 1, rad >> 1
    none = np.iinfo(np.int64).max
    best = np.full(len(ys), none, np.int64)
    for cy, cx, ok in cands:
        ok = ok & (cy >= 0) & (cy < h) & (cx >= 0) & (cx < w)
        ok[ok] = A[cy[ok], cx[ok]]
        i = np.nonzero(ok)[0]
        if len(i):
            cost = window_cost(T, W, ys[i], xs[i], cy[i], cx[i], r)
            best[i] = np.minimum(best[i], cost * (h * w) + cy[i] * w + cx[i])
    s = np.where(best == none, -1, best % (h * w))
    ny, nx = np.full((h, w), -1, np.int64), np.full((h, w), -1, np.int64)
    ny[ys, xs], nx[ys, xs] = np.where(s < 0, -1, s // w), np.where(s < 0, -1, s % w)
    return ny, nx


def image_ref(page, hole, init, radius, levels, iters, seed):
    h, w = hole.shape
    Ws, Hs = [np.where(hole[..., None], init, page).astype(np.int64)], [hole]
    sizes = [(h, w)]
    while len(sizes) < 8:
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    L = max(1, min(levels, sum(1 for a, b in sizes[:levels] if min(a, b) >= 2 * radius + 1)))
    for _ in range(L - 1):
        Wn, Hn = pull_ref(Ws[-1], Hs[-1])
        Ws.append(Wn)
        Hs.append(Hn)
    fy = fx = None
    for l in range(L - 1, -1, -1):
        W, H = Ws[l], Hs[l]
        hl, wl = H.shape
        A = admissible_ref(H, radius)
        if fy is None:
            ny, nx = np.full((hl, wl), -1, np.int64), np.full((hl, wl), -1, np.int64)
        else:
            yy, xx = np.mgrid[0:hl, 0:wl]
            psy, psx = fy[yy >> 1, xx >> 1], fx[yy >> 1, xx >> 1]
            cy, cx = 2 * psy + (yy & 1), 2 * psx + (xx & 1)
            ok = H & (psy >= 0) & (cy < hl) & (cx < wl)
            ok[ok] = A[cy[ok], cx[ok]]
            ny, nx = np.where(ok, cy, -1), np.where(ok, cx, -1)
        fy, fx = ny, nx
        for t in range(1, iters + 1):
            key = int(mix(np.uint64((seed + GOLDEN * (16 * l + t)) & 0xFFFFFFFF)))
            fy, fx = iterate_ref(W, H, A, fy, fx, radius, key)
    out = np.where(hole[..., None], init, page)
    src = hole & (fy >= 0)
    out[src] = page[fy[src], fx[src]]
    stats = [int(hole.sum()), int(src.sum()), int(hole.sum() - src.sum())]
    return out, np.stack([fy, fx], axis=-1).astype(np.int32), np.array(stats, np.int32)


def patch_ref(page, hole, init, radius, levels, iters, seed):
    parts = [image_ref(page[k], hole[k], init[k], radius, levels, iters, seed) for k in range(len(page))]
    return tuple(np.stack([p[i] for p in parts]) for i in range(3))


# ---- pages and holes -----------------------------------------------------------------------------------------------------------------
def holes_of(kind, h, w):
    m = np.zeros((h, w), bool)
    if kind == "rects":                                    # across the lines x = 31 / 32 and y = 15 / 16 of the 150 x 217 page; one noise, one lattice
        m[h // 3:h // 3 + max(1, h // 5), w // 6:w // 6 + max(1, w // 3)] = True
        m[(2 * h) // 3:(2 * h) // 3 + max(1, h // 10), w // 2:w // 2 + max(1, w // 4)] = True
        m[h // 2, (3 * w) // 4] = True
    elif kind == "one":
        m[h // 2, w // 2] = True
    elif kind == "edge":                                   # the top left corner and a run along the bottom edge to the right edge
        m[0:max(1, h // 6), 0:max(1, w // 4)] = True
        m[h - 1, w // 2:] = True
    elif kind == "full":
        m[:] = True
    return m


@functools.lru_cache(maxsize=None)
def inputs(kind, n, h, w):
    """(page [n, h, w, 3] uint8 -- different images --, hole bool [n, h, w], init random bytes): computed once; callers do not modify them"""
    rng = np.random.default_rng(100 + 7 * h + w + len(kind))
    page = np.stack([quarters_page(h, w, seed=3 + 11 * k)[:, ::(-1 if k % 2 else 1)] for k in range(n)])
    hole = np.stack([np.roll(holes_of(kind, h, w), (3 * k, 5 * k), axis=(0, 1)) for k in range(n)])
    init = rng.integers(0, 256, size=page.shape, dtype=np.uint8)
    return np.ascontiguousarray(page), hole, init


@functools.lru_cache(maxsize=None)
def reference(kind, n, h, w, radius, levels, iters, seed):
    page, hole, init = inputs(kind, n, h, w)
    return patch_ref(page, hole, init, radius, levels, iters, seed)


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------
def run(dev, page, hole, init, radius, levels, iters, seed, ws=None, **bad):
    """one call -> (out, nnf, stats, the workspace Buf); the canary tails of out, nnf, stats and ws are checked, the inputs are read only"""
    n, h, w = hole.shape
    lib = _lib.lib()
    nbytes = lib.tsii_patch_fill_ws_bytes(n, h, w, radius, levels)
    assert 0 < nbytes <= 18 * n * h * w * 4 // 3 + 16 * 5 * 6 and nbytes % 16 == 0
    pd, hd, idev = up(dev, page), up(dev, hole.astype(np.uint8) * 255), up(dev, init)
    out, nnf, stats = Buf(dev, page.size, torch.uint8), Buf(dev, 2 * hole.size, torch.int32), Buf(dev, 3 * n, torch.int32)
    ws = Buf(dev, nbytes, torch.uint8) if ws is None else ws
    a = dict(page=_lib.ptr(pd), hole=_lib.ptr(hd), init=_lib.ptr(idev), n=n, h=h, w=w, radius=radius, levels=levels, iters=iters, seed=seed,
             out=out.ptr, nnf=nnf.ptr, stats=stats.ptr, ws=ws.ptr)
    a.update(bad)
    _lib.call("tsii_patch_fill", a["page"], a["hole"], a["init"], a["n"], a["h"], a["w"], a["radius"], a["levels"], a["iters"], a["seed"],
              a["out"], a["nnf"], a["stats"], a["ws"], _lib.stream())
    got = out.get().reshape(n, h, w, 3), nnf.get().reshape(n, h, w, 2), stats.get().reshape(n, 3)
    ws.get()
    assert np.array_equal(pd.cpu().numpy(), page) and np.array_equal(idev.cpu().numpy(), init), "page and init are read only"
    return got + (ws,)


def check_by_construction(page, hole, init, out, nnf, stats, radius):
    """what holds whatever the search found"""
    n, h, w = hole.shape
    assert np.array_equal(out[~hole], page[~hole]), "valid pixels byte for byte"
    assert bool((nnf[~hole] == -1).all())
    for k in range(n):
        sy, sx = nnf[k, ..., 0], nnf[k, ..., 1]
        src = sy >= 0
        assert bool((src <= hole[k]).all()) and bool(((sx >= 0) == src).all())
        assert bool(admissible_ref(hole[k], radius)[sy[src], sx[src]].all()), "every source window lies on the page and holds no hole"
        assert np.array_equal(out[k][src], page[k][sy[src], sx[src]]), "a sourced pixel is the page pixel it names"
        rest = hole[k] & ~src
        assert np.array_equal(out[k][rest], init[k][rest]), "a hole pixel without a source keeps init"
        assert stats[k].tolist() == [int(hole[k].sum()), int(src.sum()), int(rest.sum())]


@both_backends
@pytest.mark.parametrize("params", PARAMS, **IDS)
@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_against_the_restatement(backend, shape, params):
    n, h, w = shape
    with BACKENDS[backend]() as dev:
        for kind in KINDS:
            page, hole, init = inputs(kind, n, h, w)
            out, nnf, stats, _ = run(dev, page, hole, init, *params)
            ref_out, ref_nnf, ref_stats = reference(kind, n, h, w, *params)
            assert np.array_equal(nnf, ref_nnf), (kind, int((nnf != ref_nnf).any(axis=-1).sum()))
            assert np.array_equal(out, ref_out), (kind, int((out != ref_out).any(axis=-1).sum()))
            assert np.array_equal(stats, ref_stats), (kind, stats, ref_stats)
            check_by_construction(page, hole, init, out, nnf, stats, params[0])
            if kind == "none":
                assert np.array_equal(out, page) and not stats.any()
            if kind == "full":
                assert np.array_equal(out, init) and stats[:, 1].sum() == 0, "a page that is all hole has no source"
            if kind == "rects" and (h, w) == (150, 217):
                print(f"150 x 217, rects, {params}: holes, sourced, unsourced = {stats[0].tolist()}")
                assert stats[0, 0] == 2971 and 10 * stats[0, 1] > 9 * stats[0, 0], "the search has work and finds sources"


@both_backends
@pytest.mark.parametrize("shape", SHAPES[1:], **IDS)
def test_page_under_the_holes_is_never_used(backend, shape):
    n, h, w = shape
    params = (3, 3, 3, 0) if h >= 7 else (1, 3, 3, 5)
    rng = np.random.default_rng(5)
    with BACKENDS[backend]() as dev:
        for kind in ("rects", "edge"):
            page, hole, init = inputs(kind, n, h, w)
            first = run(dev, page, hole, init, *params)[:3]
            other = page.copy()
            other[hole] = rng.integers(0, 256, size=(int(hole.sum()), 3), dtype=np.uint8)
            assert bool((other != page).any())
            second = run(dev, other, hole, init, *params)[:3]
            for a, b in zip(first, second):
                assert np.array_equal(a, b), kind


@both_backends
def test_two_runs_a_used_workspace_and_another_seed(backend):
    """the same call twice, the second time on the workspace another shape left behind: identical bits; another seed may differ and still
    holds what holds by construction"""
    page, hole, init = inputs("rects", 1, 150, 217)
    small = inputs("edge", 2, 40, 50)
    with BACKENDS[backend]() as dev:
        first = run(dev, page, hole, init, 3, 3, 3, 0)
        run(dev, *small, 4, 3, 1, 5, ws=first[3])          # a smaller problem in the same (larger) workspace
        second = run(dev, page, hole, init, 3, 3, 3, 0, ws=first[3])
        third = run(dev, page, hole, init, 3, 3, 3, 12345)
    for a, b in zip(first[:3], second[:3]):
        assert np.array_equal(a, b)
    check_by_construction(page, hole, init, *third[:3], 3)
    assert third[2][0, 1] == third[2][0, 0]


@both_backends
@pytest.mark.parametrize("hw", [(40, 50), (150, 217)], **IDS)
def test_batch_images_equal_the_image_alone(backend, hw):
    h, w = hw
    parts = [inputs(kind, 1, h, w) for kind in ("rects", "edge", "one")]
    page, hole, init = (np.concatenate([p[i] for p in parts]) for i in range(3))
    page[1] = page[1, ::-1]                                # different images
    with BACKENDS[backend]() as dev:
        together = run(dev, page, hole, init, 3, 3, 3, 5)[:3]
        alone = [run(dev, page[k:k + 1], hole[k:k + 1], init[k:k + 1], 3, 3, 3, 5)[:3] for k in range(3)]
    for k in range(3):
        for a, b in zip(together, alone[k]):
            assert np.array_equal(a[k], b[0]), k
    check_by_construction(page, hole, init, *together, 3)


@both_backends
def test_out_may_be_init(backend):
    page, hole, init = inputs("rects", 2, 40, 50)
    with BACKENDS[backend]() as dev:
        apart = run(dev, page, hole, init, 3, 3, 3, 0)[:3]
        n, h, w = hole.shape
        pd, hd = up(dev, page), up(dev, hole.astype(np.uint8))
        both = Buf(dev, init.size, torch.uint8)
        both.raw[:init.size] = up(dev, init.reshape(-1))
        nnf, stats = Buf(dev, 2 * hole.size, torch.int32), Buf(dev, 3 * n, torch.int32)
        ws = Buf(dev, _lib.lib().tsii_patch_fill_ws_bytes(n, h, w, 3, 3), torch.uint8)
        _lib.call("tsii_patch_fill", _lib.ptr(pd), _lib.ptr(hd), both.ptr, n, h, w, 3, 3, 3, 0, both.ptr, nnf.ptr, stats.ptr, ws.ptr, _lib.stream())
        inside = both.get().reshape(n, h, w, 3), nnf.get().reshape(n, h, w, 2), stats.get().reshape(n, 3)
        ws.get()
    for a, b in zip(apart, inside):
        assert np.array_equal(a, b)


@both_backends
def test_refusals(backend):
    page, hole, init = inputs("rects", 2, 40, 50)
    lib = _lib.lib
    with BACKENDS[backend]() as dev:
        size = lib().tsii_patch_fill_ws_bytes
        for n, h, w, radius, levels in ((2, 40, 50, 0, 3), (2, 40, 50, 5, 3), (2, 40, 50, 3, 0), (2, 40, 50, 3, 7), (0, 40, 50, 3, 3),
                                        (2, 0, 50, 3, 3), (2, 40, 0, 3, 3), (-1, 40, 50, 3, 3), (1, 26755, 26755, 3, 3), (2 ** 20, 2 ** 10, 1, 3, 3)):
            assert size(n, h, w, radius, levels) == 0, (n, h, w, radius, levels)
        assert size(1, 26754, 26754, 3, 3) > 0, "2^31 - 154100 elements"
        assert size(2, 40, 50, 4, 6) > 0 and size(2, 40, 50, 1, 1) > 0
        pd, hd, idev = up(dev, page), up(dev, hole.astype(np.uint8)), up(dev, init)
        left = []
        for bad in (dict(radius=0), dict(radius=5), dict(levels=0), dict(levels=7), dict(iters=0), dict(iters=9), dict(n=0), dict(h=0),
                    dict(w=0), dict(n=-2), dict(h=26755, w=26755, n=1), dict(page=None), dict(hole=None), dict(init=None), dict(out=None),
                    dict(nnf=None), dict(stats=None), dict(ws=None), dict(out=_lib.ptr(pd))):
            n, h, w = hole.shape
            out, nnf, stats = Buf(dev, page.size, torch.uint8), Buf(dev, 2 * hole.size, torch.int32), Buf(dev, 3 * n, torch.int32)
            ws = Buf(dev, size(n, h, w, 3, 3), torch.uint8)
            a = dict(page=_lib.ptr(pd), hole=_lib.ptr(hd), init=_lib.ptr(idev), n=n, h=h, w=w, radius=3, levels=3, iters=3, seed=0, out=out.ptr,
                     nnf=nnf.ptr, stats=stats.ptr, ws=ws.ptr)
            a.update(bad)
            with pytest.raises(RuntimeError, match=r"tsii_patch_fill failed \(-?[1-9]\d*\): patch_fill: "):
                _lib.call("tsii_patch_fill", a["page"], a["hole"], a["init"], a["n"], a["h"], a["w"], a["radius"], a["levels"], a["iters"],
                          a["seed"], a["out"], a["nnf"], a["stats"], a["ws"], _lib.stream())
            left.append((out.get(), nnf.get(), stats.get(), ws.get()))
        page_after = pd.cpu().numpy()
    for bufs in left:
        assert all(bool((b.view(np.uint8) == 0xA5).all()) for b in bufs), "a refused call launches nothing"
    assert np.array_equal(page_after, page)
