"""Text regions (csrc/regions.hip, include/tsii_hip.h "K10: text regions"): connected-component labelling, areas, boxes, the
minimum-area filter and the per-tile core counts, through the C ABI on the emulator (CPU suite) and, with -m gpu, on the chip; then
``text_regions`` and the ``TextEraser`` options built on them.

Everything is integer: every comparison is EQUALITY with the restatement below, which does not share the kernels' algorithm.  It starts
from ``idx + 1`` on the foreground and repeats "minimum over the foreground neighbours" until nothing changes (between two rounds every
pixel also takes the value of the pixel its value names -- a pixel of its own component, so the fixed point is the same and a chain of
n pixels settles in about log n rounds instead of n); areas and boxes come from ``np.unique`` / ``np.bincount``.  Every output buffer,
the text plane and the workspace carry a canary tail; the workspace is handed over full of canary bytes (nothing has to be cleared).
"""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import text_segmentation_image_inpainting_amd as T
from tests.backends import BACKENDS, both_backends
from tests.test_pipeline_kernels import CANARY, Buf
from text_segmentation_image_inpainting_amd import _lib
from text_segmentation_image_inpainting_amd.masks import MaskParts
from text_segmentation_image_inpainting_amd.pipeline import tile_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, HALO = 64, 8
PAGES = [(1, 1), (5, 217), (40, 50), (150, 217), (300, 420)]      # the last: several 64 x 32 blocks meet in both directions
BIG = [(150, 217), (300, 420)]
CANARY32 = int(np.frombuffer(bytes([CANARY] * 4), np.int32)[0])


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def components(fg, connectivity):
    """int64 [h,w]: 1 + the smallest pixel index of each pixel's component, 0 on the background"""
    h, w = fg.shape
    big = np.int64(h * w + 1)
    lab = np.where(fg, np.arange(1, h * w + 1, dtype=np.int64).reshape(h, w), big)
    steps = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])
    while True:
        pad = np.pad(lab, 1, constant_values=big)
        new = lab
        for dy, dx in steps + [(-dy, -dx) for dy, dx in steps]:
            new = np.minimum(new, pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w])
        new = np.where(fg, new, big)
        new = np.where(fg, np.minimum(new, np.append(new.reshape(-1), big)[np.minimum(new, big) - 1].reshape(h, w)), big)
        if np.array_equal(new, lab):
            return np.where(fg, lab, 0)
        lab = new


def expected(text, connectivity, min_area, g):
    """-> dict(labels, text, n, table (every kept row), core)"""
    h, w = text.shape
    full = components(text != 0, connectivity)
    ids, area = np.unique(full[full > 0], return_counts=True)
    assert np.array_equal(area, np.bincount(full.reshape(-1), minlength=h * w + 1)[ids])
    kept = ids[area >= min_area]
    labels = np.where(np.isin(full, kept), full, 0)
    ys, xs = np.nonzero(labels)
    _, inv = np.unique(labels[ys, xs], return_inverse=True)          # ascending label order: row k belongs to kept[k]
    y0, x0, y1, x1 = (np.full(len(kept), v, np.int64) for v in (h, w, 0, 0))
    np.minimum.at(y0, inv, ys), np.minimum.at(x0, inv, xs), np.maximum.at(y1, inv, ys + 1), np.maximum.at(x1, inv, xs + 1)
    rows = np.stack([kept, area[area >= min_area], y0, x0, y1, x1], axis=1) if len(kept) else []
    out = (labels != 0).astype(np.uint8)
    core = None if g is None else np.array([out[y0:y1, x0:x1].sum() for (y0, y1, x0, x1) in map(g.core, range(g.count))], np.int32)
    return dict(labels=labels.astype(np.int32), text=out, n=(len(ids), len(kept)), table=np.array(rows, np.int32).reshape(-1, 6), core=core)


# ---- patterns --------------------------------------------------------------------------------------------------------------------
def pattern(name, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    if name.startswith("noise"):
        p = float(name[5:])
        return (np.random.default_rng(int(p * 100) + h).random((h, w)) < p).astype(np.uint8) * 3     # bytes 0 / 3: non-zero is text
    if name == "full":
        return np.full((h, w), 255, np.uint8)
    if name == "empty":
        return np.zeros((h, w), np.uint8)
    if name == "checker":
        return ((yy + xx) % 2 == 0).astype(np.uint8)
    if name == "serpentine":        # full rows on every second line, joined alternately at the right and left ends
        t = (yy % 2 == 0)
        t |= (yy % 4 == 1) & (xx == w - 1)
        t |= (yy % 4 == 3) & (xx == 0)
        return t.astype(np.uint8)
    if name == "staircase":         # one-pixel anti-diagonal (wrapping on pages taller than wide)
        return (xx == (w - 1 - yy) % w).astype(np.uint8)
    if name == "comb":              # teeth one background column apart, joined only by a spine in the last row
        return (((xx % 2 == 0) & (yy < h - 1)) | (yy == h - 1)).astype(np.uint8)
    if name == "comb_up":           # mirrored: the spine is the first row, the smallest index lies in it
        return (((xx % 2 == 0) & (yy > 0)) | (yy == 0)).astype(np.uint8)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name, h, w, connectivity, min_area=0, tiled=True):
    """(text, expectation): computed once, shared by the backends; callers do not modify it"""
    text = pattern(name, h, w)
    g = tile_grid(h, w, TILE, HALO) if tiled else None
    return text, expected(text, connectivity, min_area, g)


# ---- the kernels -----------------------------------------------------------------------------------------------------------------
class Planes:
    """the buffers of one call, every one with a canary tail; the text plane's payload is the input"""

    def __init__(self, dev, text, max_regions, g):
        h, w = text.shape
        self.h, self.w, self.g, self.max_regions = h, w, g, max_regions
        self.text = Buf(dev, h * w, torch.uint8)
        self.text.raw[:h * w] = torch.from_numpy(np.ascontiguousarray(text).reshape(-1)).to(dev)
        self.labels, self.n = Buf(dev, h * w, torch.int32), Buf(dev, 2, torch.int32)
        self.table = Buf(dev, 6 * max_regions, torch.int32) if max_regions else None
        self.core = Buf(dev, g.count, torch.int32) if g is not None else None
        nbytes = _lib.lib().tsii_text_regions_ws_bytes(h, w, max_regions)
        assert nbytes > 0 and nbytes % 4 == 0
        self.ws = Buf(dev, nbytes // 4, torch.int32)

    def run(self, connectivity, min_area, tile=TILE, halo=HALO):
        _lib.call("tsii_text_regions", self.text.ptr, self.h, self.w, connectivity, min_area, self.max_regions, tile, halo,
                  self.core.ptr if self.core else None, self.labels.ptr, self.table.ptr if self.table else None, self.n.ptr,
                  self.ws.ptr, _lib.stream())

    def get(self):
        self.ws.get()                                    # the canary behind the workspace
        return dict(labels=self.labels.get().reshape(self.h, self.w), text=self.text.get().reshape(self.h, self.w), n=tuple(self.n.get()),
                    table=self.table.get().reshape(-1, 6) if self.table else np.zeros((0, 6), np.int32),
                    core=self.core.get() if self.core else None)


def check(got, exp, max_regions):
    assert got["n"] == exp["n"], (got["n"], exp["n"])
    assert np.array_equal(got["labels"], exp["labels"]), int((got["labels"] != exp["labels"]).sum())
    assert np.array_equal(got["text"], exp["text"])
    n = min(exp["n"][1], max_regions)
    assert np.array_equal(got["table"][:n], exp["table"][:n])
    assert bool((got["table"][n:] == CANARY32).all()), "rows behind the kept regions must not be touched"
    if exp["core"] is not None:
        assert np.array_equal(got["core"], exp["core"]), (got["core"], exp["core"])


def run_case(backend, name, hw, connectivity, min_area=0, max_regions=None, tiled=True):
    text, exp = case(name, *hw, connectivity, min_area, tiled)
    max_regions = exp["n"][1] + 3 if max_regions is None else max_regions
    with BACKENDS[backend]() as dev:
        planes = Planes(dev, text, max_regions, tile_grid(*hw, TILE, HALO) if tiled else None)
        planes.run(connectivity, min_area)
        got = planes.get()
    check(got, exp, max_regions)
    return exp


IDS = dict(ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else str(v))


@both_backends
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", ["noise0.3", "noise0.45", "noise0.6", "full", "empty", "checker", "staircase"])
@pytest.mark.parametrize("hw", PAGES, **IDS)
def test_patterns(backend, hw, name, connectivity):
    exp = run_case(backend, name, hw, connectivity)
    h, w = hw
    if name == "full":
        assert exp["n"] == (1, 1) and tuple(exp["table"][0]) == (1, h * w, 0, 0, h, w)
    if name == "empty":
        assert exp["n"] == (0, 0) and not exp["core"].any()
    if name == "checker":
        assert exp["n"][0] == (1 if connectivity == 8 or h * w == 1 else (h * w + 1) // 2)
    if name == "staircase" and h <= w:
        assert exp["n"][0] == (1 if connectivity == 8 else h)


@both_backends
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", ["serpentine", "comb", "comb_up"])
@pytest.mark.parametrize("hw", BIG, **IDS)
def test_chains_through_every_block(backend, hw, name, connectivity):
    """one component whose merge chain passes through every block (serpentine), or whose parts meet only in other blocks (combs)"""
    exp = run_case(backend, name, hw, connectivity)
    assert exp["n"] == (1, 1) and exp["table"][0][0] == 1


@both_backends
def test_truncated_table(backend):
    """16275 singletons, room for 100: exactly the first 100 rows in raster order, the rows behind them untouched, the true count"""
    exp = run_case(backend, "checker", (150, 217), 4, max_regions=100)
    assert exp["n"] == (16275, 16275)
    assert np.array_equal(exp["table"][:100, 0], 1 + 2 * np.arange(100))
    run_case(backend, "checker", (150, 217), 4, max_regions=0)         # no table at all (table == NULL)


@both_backends
@pytest.mark.parametrize("tiled", [True, False], ids=["core_count", "no_core_count"])
@pytest.mark.parametrize("min_area", [0, 1, 2, 5, 50, 150 * 217 + 1])
@pytest.mark.parametrize("connectivity", [4, 8])
def test_min_area(backend, connectivity, min_area, tiled):
    exp = run_case(backend, "noise0.45", (150, 217), connectivity, min_area, tiled=tiled)
    found, kept = exp["n"]
    assert found > 100 and (kept == found if min_area <= 1 else kept < found) and (kept > 0 or min_area > 50)


@both_backends
def test_same_workspace_twice(backend):
    """the second call reuses the first call's workspace as it was left: identical outputs"""
    text, exp = case("noise0.45", 150, 217, 8, 5)
    with BACKENDS[backend]() as dev:
        a = Planes(dev, text, 4096, tile_grid(150, 217, TILE, HALO))
        a.run(8, 5)
        first = a.get()
        b = Planes(dev, text, 4096, a.g)
        b.ws = a.ws
        b.run(8, 5)
        second = b.get()
    check(first, exp, 4096)
    check(second, exp, 4096)


@both_backends
def test_refusals(backend):
    text = pattern("noise0.45", 40, 50)
    with BACKENDS[backend]() as dev:
        assert _lib.lib().tsii_text_regions_ws_bytes(46341, 46341, 1) == 0
        assert _lib.lib().tsii_text_regions_ws_bytes(0, 5, 1) == 0 and _lib.lib().tsii_text_regions_ws_bytes(5, 5, -1) == 0
        p = Planes(dev, text, 16, tile_grid(40, 50, TILE, HALO))
        with pytest.raises(RuntimeError, match=r"tsii_text_regions failed \(-?[1-9]\d*\): .*connectivity"):
            p.run(6, 0)
        with pytest.raises(RuntimeError, match="geometry"):
            p.run(8, 0, tile=48, halo=4)
        with pytest.raises(RuntimeError, match="geometry"):
            p.run(8, 0, tile=64, halo=32)
        p.max_regions = -1
        with pytest.raises(RuntimeError, match="max_regions"):
            p.run(8, 0)
        got = p.get()
        ws = p.ws.get()
    assert np.array_equal(got["text"], text), "a refused call must not touch the text plane"
    for name in ("labels", "n", "table", "core"):
        assert bool((np.asarray(got[name]) == CANARY32).all()), name
    assert bool((ws == CANARY32).all())


def test_restatement_against_scipy():
    """CPU suite only: the restatement's partition is scipy's"""
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, hw in (("noise0.45", (150, 217)), ("noise0.6", (40, 50)), ("serpentine", (150, 217)), ("comb_up", (150, 217))):
        for connectivity in (4, 8):
            text, exp = case(name, *hw, connectivity)
            lab, n = ndimage.label(text != 0, structure=np.ones((3, 3)) if connectivity == 8 else None)
            assert n == exp["n"][0]
            pairs = np.unique(np.stack([lab.reshape(-1), exp["labels"].reshape(-1)]), axis=1)
            assert pairs.shape[1] == n + (1 if (text == 0).any() else 0), "the two partitions differ"


# ---- text_regions ----------------------------------------------------------------------------------------------------------------
@both_backends
def test_text_regions_api(backend):
    text, exp = case("noise0.45", 150, 217, 8, 5, False)
    mask = (text != 0).astype(np.uint8) * 255                        # what TextEraser returns
    keep = mask.copy()
    with BACKENDS[backend]() as dev:
        r = T.text_regions(mask, min_area=5, device=dev)
        t_in = torch.from_numpy(mask).to(dev)
        rt = T.text_regions(t_in, connectivity=8, min_area=5, max_regions=7, device=dev)
        r4 = T.text_regions(mask, connectivity=4, device=dev)
        assert torch.equal(t_in.cpu(), torch.from_numpy(keep)), "the argument must not be modified"
        assert isinstance(rt.labels, torch.Tensor) and rt.labels.device == t_in.device and rt.labels.dtype == torch.int32
        rt_labels = rt.labels.cpu().numpy()
    assert np.array_equal(mask, keep)
    assert isinstance(r, T.TextRegions) and isinstance(r.labels, np.ndarray) and r.labels.dtype == np.int32
    assert np.array_equal(r.labels, exp["labels"]) and np.array_equal(r.table, exp["table"])
    assert (r.found, r.kept, r.truncated) == (exp["n"][0], exp["n"][1], False) and r.table.dtype == np.int32
    assert np.array_equal(rt_labels, exp["labels"]) and np.array_equal(rt.table, exp["table"][:7])
    assert (rt.found, rt.kept, rt.truncated) == (exp["n"][0], exp["n"][1], True)
    exp4 = case("noise0.45", 150, 217, 4, 0, False)[1]
    assert np.array_equal(r4.labels, exp4["labels"]) and r4.kept == r4.found == exp4["n"][0] and not r4.truncated
    assert np.array_equal(r4.table, exp4["table"])


def test_arguments_are_checked():
    mask = np.zeros((4, 4), np.uint8)
    for kw in (dict(connectivity=6), dict(min_area=-1), dict(max_regions=0), dict(min_area=2.5)):
        with pytest.raises(ValueError):
            T.text_regions(mask, **kw)
        with pytest.raises(ValueError):
            T.TextEraser(lambda x: x, lambda x: x, device="cpu", **kw)
    with pytest.raises(ValueError, match="uint8"):
        T.text_regions(np.zeros((4, 4), np.float32))


# ---- TextEraser: stand-in nets (fixed sequences of shifted adds, radius R <= halo: the same arithmetic at any tensor size) ------------
MEAN, STD = (0.4935, 0.4563, 0.4544), (0.3769, 0.3615, 0.3566)
R = 4
TAPS = [(0, 0), (-R, 0), (0, R), (2, -3)]


def shifted(x, dy, dx):
    h, w = x.shape[-2:]
    return F.pad(x, (R, R, R, R))[..., R + dy:R + dy + h, R + dx:R + dx + w]


def standin_segmenter(x):
    acc = shifted(x[:, 0:1], *TAPS[0]) * 0.5 + shifted(x[:, 1:2], *TAPS[1]) * 0.25
    acc = acc + shifted(x[:, 2:3], *TAPS[2]) * 0.25
    return -(acc + 0.4)                                  # dark ink -> positive logit


def standin_filler(args):
    x, mask = args
    m = (mask.as_tensor() if isinstance(mask, MaskParts) else mask)[:, :1]
    num, den = shifted(x, *TAPS[0]), shifted(m, *TAPS[0])
    for tap in TAPS[1:]:
        num, den = num + shifted(x, *tap), den + shifted(m, *tap)
    return num / den.clamp(min=1.0)


def reflect(v, n):
    p = 2 * (n - 1)
    v = np.mod(np.asarray(v), p)
    return np.where(v < n, v, p - v)


def whole_page(page, halo, dilate, connectivity, min_area, dev):
    """the stand-ins applied once to the whole page, the region filter between the dilation and the filler"""
    h, w = page.shape[:2]
    mean, std = np.asarray(MEAN, np.float32), np.asarray(STD, np.float32)
    scale, shift = np.float32(1.0) / (np.float32(255.0) * std), -mean / std
    xn = (page.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)).astype(np.float32)      # fmaf: one rounding
    ext = xn[reflect(np.arange(-halo, h + halo), h)][:, reflect(np.arange(-halo, w + halo), w)]
    logits = standin_segmenter(torch.from_numpy(ext).to(dev).permute(2, 0, 1)[None])[0, 0, halo:halo + h, halo:halo + w].cpu().numpy()
    t = torch.from_numpy((logits > np.float32(0.0)).astype(np.float32))[None, None]
    dilated = F.max_pool2d(t, dilate, 1, dilate // 2)[0, 0].numpy().astype(np.uint8)
    exp = expected(dilated, connectivity, min_area, None)
    text = exp["text"]
    m = np.zeros((h + 2 * halo, w + 2 * halo), np.float32)
    m[halo:halo + h, halo:halo + w] = 1 - text
    x = np.zeros((h + 2 * halo, w + 2 * halo, 3), np.float32)
    x[halo:halo + h, halo:halo + w] = page.astype(np.float32) / np.float32(255.0)
    x = x * m[..., None]
    out = standin_filler((torch.from_numpy(x).to(dev).permute(2, 0, 1)[None], torch.from_numpy(m).to(dev)[None, None]))
    out = out[0, :, halo:halo + h, halo:halo + w].permute(1, 2, 0).cpu().numpy()
    c = np.clip(out.astype(np.float32), np.float32(0), np.float32(1)).astype(np.float64)
    byte = np.floor((c * 255.0 + 0.5).astype(np.float32)).astype(np.uint8)
    return np.where(text[..., None] > 0, byte, page), dilated, exp


def fill_planes(text, g, ids):
    mask = np.zeros((len(ids), g.tile, g.tile), np.float32)
    for k, t in enumerate(ids):
        oy, ox = g.origin(t)
        ys, xs = oy + np.arange(g.tile), ox + np.arange(g.tile)
        iy, ix = np.nonzero((ys >= 0) & (ys < g.h))[0], np.nonzero((xs >= 0) & (xs < g.w))[0]
        mask[k][np.ix_(iy, ix)] = (1 - text[ys[iy]][:, xs[ix]]).astype(np.float32)
    return mask


@both_backends
def test_eraser_drops_small_regions(backend):
    tile, halo, dilate, tile_batch = 64, 16, 3, 3
    h, w = 100, 150
    g = tile_grid(h, w, tile, halo)
    s = g.stride
    rng = np.random.default_rng(21)
    page = rng.integers(200, 256, size=(h, w, 3), dtype=np.uint8)
    page[s - 6:s + 7, s - 9:s + 8] = rng.integers(0, 40, size=(13, 17, 3), dtype=np.uint8)       # large, across a core boundary
    page[2 * s + 12:2 * s + 20, 3 * s + 10:3 * s + 18] = rng.integers(0, 40, size=(8, 8, 3), dtype=np.uint8)   # small, alone in its tile
    small_tile = 2 * g.tx + 3
    calls = []

    def spy(args):
        calls.append(args[1].parts[0].plane.detach().cpu().numpy().copy())
        return standin_filler(args)

    with BACKENDS[backend]() as dev:
        _, dilated, unfiltered = whole_page(page, halo, dilate, 8, 0, dev)
        areas = sorted(unfiltered["table"][:, 1])
        assert len(areas) == 2 and areas[0] < areas[1], areas
        min_area = (areas[0] + areas[1]) // 2 + 1                      # between the two dilated areas
        clean_ref, _, exp = whole_page(page, halo, dilate, 8, min_area, dev)
        eraser = T.TextEraser(standin_segmenter, spy, mean=MEAN, std=STD, tile=tile, halo=halo, dilate=dilate, tile_batch=tile_batch,
                              device=dev, min_area=min_area)
        clean, mask = eraser(page)
        labels = eraser.last_labels.cpu().numpy()
        boxes_only = T.TextEraser(standin_segmenter, standin_filler, mean=MEAN, std=STD, tile=tile, halo=halo, dilate=dilate, device=dev,
                                  regions=True, connectivity=4, max_regions=1)
        clean_all, mask_all = boxes_only(page)
    text_ref = exp["text"]
    assert np.array_equal(mask, text_ref * 255) and np.array_equal(clean, clean_ref), int((clean != clean_ref).sum())
    assert np.array_equal(labels, exp["labels"])
    counts = [int(text_ref[y0:y1, x0:x1].sum()) for (y0, y1, x0, x1) in map(g.core, range(g.count))]
    selected = [t for t in range(g.count) if counts[t] > 0]
    y0, y1, x0, x1 = g.core(small_tile)
    assert dilated[y0:y1, x0:x1].sum() == areas[0] and small_tile not in selected and len(selected) > 1
    assert np.array_equal(np.concatenate(calls), fill_planes(text_ref, g, selected)), "the filler saw exactly the tiles of the kept region"
    assert np.array_equal(clean[y0:y1, x0:x1], page[y0:y1, x0:x1]) and not mask[y0:y1, x0:x1].any()
    assert bool(text_ref[:, s - 1].any() and text_ref[:, s].any() and text_ref[s - 1].any() and text_ref[s].any())
    assert eraser.last_stats == {"tiles": g.count, "selected": len(selected), "text_pixels": int(text_ref.sum())}
    reg = eraser.last_regions
    assert sorted(reg) == ["found", "kept", "table", "truncated"] and (reg["found"], reg["kept"], reg["truncated"]) == (2, 1, False)
    assert np.array_equal(reg["table"], exp["table"]) and reg["table"].dtype == np.int32
    # regions=True without a filter: the page's result is the unfiltered one, the table is cut at max_regions
    assert np.array_equal(mask_all, dilated * 255) and boxes_only.last_stats["text_pixels"] == int(dilated.sum())
    r = boxes_only.last_regions
    assert (r["found"], r["kept"], r["truncated"]) == (2, 2, True) and np.array_equal(r["table"], expected(dilated, 4, 0, None)["table"][:1])


@both_backends
def test_default_eraser_never_labels(backend, monkeypatch):
    from text_segmentation_image_inpainting_amd import pipeline, regions
    names = []
    real = _lib.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)

    page = np.random.default_rng(3).integers(0, 256, size=(70, 45, 3), dtype=np.uint8)
    with BACKENDS[backend]() as dev:
        for mod in (_lib, pipeline, regions):
            monkeypatch.setattr(mod, "call", spy)
        eraser = T.TextEraser(standin_segmenter, standin_filler, tile=64, halo=16, device=dev)
        eraser(page)
        assert "tsii_tiles_text_mask" in names and "tsii_text_regions" not in names
        assert eraser.last_regions is None and sorted(eraser.last_stats) == ["selected", "text_pixels", "tiles"]
        T.TextEraser(standin_segmenter, standin_filler, tile=64, halo=16, device=dev, min_area=1)(page)     # keeps everything: still off
        assert "tsii_text_regions" not in names
        T.TextEraser(standin_segmenter, standin_filler, tile=64, halo=16, device=dev, min_area=2)(page)
        assert "tsii_text_regions" in names


# ---- the example -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_erase_text_example_boxes_gpu(tmp_path):
    from PIL import Image
    spec = importlib.util.spec_from_file_location("erase_text", os.path.join(ROOT, "examples", "erase_text.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    with BACKENDS["gpu"]():
        demo.main(["--synthetic", "--synthetic-size", "300", "420", "--tile", "256", "--halo", "32", "--min-area", "20", "--boxes",
                   "--out-folder", str(tmp_path)])
    page = np.asarray(Image.open(tmp_path / "synthetic.png").convert("RGB"))
    clean = np.asarray(Image.open(tmp_path / "synthetic_clean.png").convert("RGB"))
    mask = np.asarray(Image.open(tmp_path / "synthetic_mask.png"))
    boxes = np.asarray(Image.open(tmp_path / "synthetic_boxes.png").convert("RGB"))
    assert page.shape == (300, 420, 3) and clean.shape == page.shape and boxes.shape == page.shape and mask.shape == page.shape[:2]
    assert set(np.unique(mask)) <= {0, 255}
    assert np.array_equal(clean[mask == 0], page[mask == 0])
    regions = T.text_regions(mask)
    assert regions.found == 0 or int(regions.table[:, 1].min()) >= 20, "no region below --min-area survives in the mask"
