"""``TextEraser(segmenter, T.HarmonicFill())``: the page pipeline with the harmonic fill (fill.py, "K14: harmonic fill") in the filler's
place -- no inpainting net.  Everything in front of the filler and behind it is what the net path runs, so the mask, the tile selection
and the statistics must be those of a run with a stand-in net, and ``clean`` must be the restated pipeline: the filler tiles as
``tsii_page_tiles_fill`` (or, packed, ``tsii_page_windows_fill``) defines them, the float64 restatement of
``tests/test_harmonic_kernels.py`` per tile, the compose rule per owning tile.  Ramp pages with drawn text, tiles of 96 with a halo of
16; every case runs on the emulator (CPU suite) and, with -m gpu, on the chip.
"""
import numpy as np
import pytest
import torch

import text_segmentation_image_inpainting_amd as T
from tests.backends import BACKENDS, both_backends
from tests.test_fill_windows_kernels import ref_compose_windows, ref_windows_fill
from tests.test_flat_kernels import flat_ref
from tests.test_harmonic_kernels import harmonic_ref
from tests.test_region_hulls import fill_hulls
from tests.test_text_eraser import MEAN, STD, core_counts, dilate_np, fill_tiles, normalise, stitch, to_byte
from tests.test_text_eraser_working_resolution import standin_filler, standin_segmenter
from tests.test_text_regions import expected
from text_segmentation_image_inpainting_amd.pipeline import tile_grid

H, W, TILE, HALO, DILATE, MAXR, SWEEPS = 200, 260, 96, 16, 3, 32, 8       # 4 x 5 tiles with cores of 64 pixels
BUBBLE = (235, 240, 200)


def ramp():
    yy, xx = np.mgrid[0:H, 0:W]
    r = 0.3 * xx / W + 0.1 * yy / H
    return np.stack([0.55 + r, 0.95 - r, 0.6 + 0.8 * r], axis=-1)


def make_page(kind):
    """a bright ramp with dark blocks that touch no tile edge (the lines 48, 79, 112, 143, ... of the page): "ramp": one block across
    the corner of four tile cores and a wide one inside a core; "bubble": the wide one and a block on a disc of one colour; "blank"""
    rng = np.random.default_rng(77)
    page = to_byte(ramp().astype(np.float32))
    dark = lambda shape: rng.integers(0, 40, size=shape + (3,), dtype=np.uint8)
    if kind != "blank":
        page[90:100, 147:174] = dark((10, 27))
    if kind == "ramp":
        page[58:70, 57:71] = dark((12, 14))
    if kind == "bubble":
        yy, xx = np.mgrid[0:H, 0:W]
        page[(yy - 150) ** 2 + (xx - 90) ** 2 <= 20 * 20] = BUBBLE
        page[146:155, 83:98] = dark((9, 15))
    return page


def restated(page, hull=False, pack=False, flat=None):
    """-> dict: clean, mask (0 / 255), rest (the plane the filler sees, 0 / 1), the number of filler tiles, the flat rows"""
    g = tile_grid(H, W, TILE, HALO)
    logits = standin_segmenter(torch.from_numpy(normalise(page)).permute(2, 0, 1)[None])[0, 0].numpy()
    final = dilate_np(logits > np.float32(0.0), DILATE)
    src, rows, exp = page, None, None
    if hull or pack or flat is not None:
        exp = expected(final, 8, 0, g)
        if hull:
            final, _ = fill_hulls(exp["text"], exp["labels"], exp["table"], min(exp["n"][1], MAXR))
            exp = expected(final, 8, 0, g)
    rest = final
    if flat is not None:
        src, rest, _, rows = flat_ref(page, final, exp["labels"], exp["table"], exp["n"][1], 3, flat)
    counts = core_counts(rest, g)
    ids = [t for t in range(g.count) if counts[t] > 0]
    clean, tiles = src.copy(), len(ids)
    if ids and pack:
        origins, rects = T.plan_fill_windows(exp["table"][:, 2:6], H, W, TILE, HALO)
        assert len(origins) < len(ids)
        img, mplane = ref_windows_fill(src, rest, TILE, origins)
        out = np.stack([harmonic_ref(img[k], mplane[k] != 0, SWEEPS) for k in range(len(img))])
        clean, tiles = ref_compose_windows(src, rest, out, origins, rects)[0], len(origins)
    elif ids:
        img, mplane = fill_tiles(src, rest, g, ids)
        for k in range(len(ids)):                          # the page is drawn so that no hole inside the page touches a tile edge
            inside = np.zeros((TILE, TILE), bool)
            oy, ox = g.origin(ids[k])
            inside[max(-oy, 0):H - oy, max(-ox, 0):W - ox] = True
            ring = np.ones((TILE, TILE), bool)
            ring[1:-1, 1:-1] = False
            assert not ((mplane[k] == 0) & inside & ring).any()
        out = np.stack([harmonic_ref(img[k], mplane[k] != 0, SWEEPS) for k in range(len(ids))])
        clean = np.where(rest[..., None] > 0, to_byte(stitch(out, g, ids)), src)
    return dict(clean=clean, mask=final * 255, rest=rest, tiles=tiles, selected=len(ids), rows=rows)


def erase(dev, page, filler=None, **kw):
    calls = []
    fill = T.HarmonicFill(SWEEPS) if filler is None else filler

    def spy(args):
        calls.append(int(args[0].shape[0]))
        return fill(args)

    eraser = T.TextEraser(standin_segmenter, spy, mean=MEAN, std=STD, tile=TILE, halo=HALO, dilate=DILATE, tile_batch=3, device=dev,
                          max_regions=MAXR, **kw)
    clean, mask = eraser(page)
    return clean, mask, eraser, calls


def check_clean(clean, mask, page, ref, on_ramp):
    """``on_ramp``: bool plane of the text pixels whose surroundings are the ramp"""
    assert np.array_equal(mask, ref["mask"]), int((mask != ref["mask"]).sum())
    assert np.array_equal(clean[mask == 0], page[mask == 0]), "clean equals the page outside the mask"
    diff = np.abs(clean.astype(int) - ref["clean"].astype(int))
    assert int(diff.max()) <= 1, "within one grey level of the restated pipeline (a float next to a .5 tie may round either way)"
    assert on_ramp.any() and bool((mask[on_ramp] == 255).all())
    off = np.abs(clean.astype(int) - to_byte(ramp().astype(np.float32)).astype(int))[on_ramp]
    assert int(off.max()) <= 2, "within two grey levels of the ramp"
    assert bool((clean[on_ramp].min(axis=-1) > 100).all()), "the dark text is gone"


@both_backends
@pytest.mark.parametrize("variant", ["plain", "pack", "hull", "flat0"])
def test_harmonic_filler_equals_the_restated_pipeline(backend, variant):
    kw = {"plain": {}, "pack": dict(pack=True), "hull": dict(hull=True), "flat0": dict(flat=0)}[variant]
    page = make_page("ramp")
    ref = restated(page, hull=variant == "hull", pack=variant == "pack", flat=0 if variant == "flat0" else None)
    with BACKENDS[backend]() as dev:
        clean, mask, eraser, calls = erase(dev, page, **kw)
        net_clean, net_mask, net_eraser, net_calls = erase(dev, page, filler=standin_filler, **kw)
    assert np.array_equal(mask, net_mask), "the mask is what the net path returns"
    assert eraser.last_stats == net_eraser.last_stats and calls == net_calls
    assert eraser.last_stats["selected"] == ref["tiles"] == sum(calls)      # packed: the windows, else the selected tiles of the grid
    if variant == "plain":
        assert ref["selected"] == 5 and calls == [3, 2]    # the corner block: four cores; the wide one: one
    if variant == "pack":
        assert eraser.last_stats["packed"] and eraser.last_stats["windows"] == 2 and eraser.last_stats["grid_selected"] == ref["selected"] == 5
    if variant == "flat0":                                 # a ramp is never flat at tolerance 0: everything reaches the filler
        assert ref["rows"][:, 0].tolist() == [0, 0] and eraser.last_stats["flat_regions"] == 0 and ref["selected"] == 5
    check_clean(clean, mask, page, ref, ref["mask"] > 0)
    assert bool((net_clean != clean).any())


@both_backends
def test_flat_sends_only_the_ramp_region(backend):
    """flat=8: the block in the bubble is painted with the bubble's colour and never reaches the filler; the one on the ramp does"""
    page = make_page("bubble")
    ref = restated(page, flat=8)
    assert ref["rows"][:, 0].tolist() == [0, 1] and ref["rows"][1, 1:4].tolist() == list(BUBBLE) and ref["selected"] == 1
    with BACKENDS[backend]() as dev:
        clean, mask, eraser, calls = erase(dev, page, flat=8)
    assert calls == [1] and eraser.last_stats["selected"] == 1 and eraser.last_stats["flat_regions"] == 1
    on_ramp = (ref["mask"] > 0) & (np.arange(H)[:, None] < 120)
    check_clean(clean, mask, page, ref, on_ramp)
    in_bubble = (ref["mask"] > 0) & ~on_ramp
    assert in_bubble.any() and bool((clean[in_bubble] == BUBBLE).all())


@both_backends
def test_blank_page_and_a_list_of_pages(backend):
    page, blank = make_page("ramp"), make_page("blank")
    ref = restated(page)
    with BACKENDS[backend]() as dev:
        clean_b, mask_b, eraser, calls = erase(dev, blank)
        assert calls == [] and eraser.last_stats == {"tiles": 20, "selected": 0, "text_pixels": 0}
        eraser = T.TextEraser(standin_segmenter, T.HarmonicFill(SWEEPS), mean=MEAN, std=STD, tile=TILE, halo=HALO, dilate=DILATE, device=dev)
        (clean_t, mask_t), (clean_n, mask_n) = eraser([torch.from_numpy(page), blank])
    assert np.array_equal(clean_b, blank) and not mask_b.any() and np.array_equal(clean_n, blank) and not mask_n.any()
    assert isinstance(clean_t, torch.Tensor) and isinstance(clean_n, np.ndarray)
    check_clean(clean_t.numpy(), mask_t.numpy(), page, ref, ref["mask"] > 0)
