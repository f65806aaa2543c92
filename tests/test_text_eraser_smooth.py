"""``TextEraser(smooth=T)``: text regions whose surroundings are locally smooth are filled harmonically at page level on the device and
never reach the filler; the route order is flat, then smooth, then the net.

Stand-in nets for which tiling cannot matter (the per-pixel segmenter and the constant-colour filler of
``tests/test_text_eraser_working_resolution.py``), so the tiled run must be EQUAL to a whole-page restatement: ``whole_page`` of
``tests/test_text_eraser_hull.py`` up to the final text plane, ``flat_fill_regions`` on it, the smooth decision of
``tests/test_smooth_kernels.py`` (per region: dilation, minus the text, shifted differences) on what is left, ``harmonic_fill`` of the
painted page over all of that, then the filler's colour on the rest.  Every case runs on the emulator (CPU suite) and, with -m gpu, on
the chip.
"""
import numpy as np
import pytest
import torch

import text_segmentation_image_inpainting_amd as T
from tests.backends import BACKENDS, both_backends
from tests.test_fill_windows_kernels import ref_windows_fill
from tests.test_smooth_kernels import smooth_ref
from tests.test_text_eraser import MEAN, STD, core_counts, fill_tiles, to_byte
from tests.test_text_eraser_flat import spied_run
from tests.test_text_eraser_hull import whole_page
from tests.test_text_eraser_working_resolution import COLOUR, DILATE, HALO, LONG, TILE, standin_filler, standin_segmenter
from tests.test_text_regions import expected
from text_segmentation_image_inpainting_amd.pipeline import tile_grid

H, W = 150, 217                                           # 4 x 5 tiles with cores of 48 pixels
TOL, RING, MAXR = 8, 3, 32
DISC = (90, 160, 230)
FILL = to_byte(np.asarray(COLOUR, np.float32))
SMOOTH_TILE, NEIGHBOUR_TILE = 10, 11                      # the core (96..144, 0..48) holds the smooth block and nothing else; 11 is to its right
VARIANTS = {"plain": {}, "hull": dict(hull=True), "pack": dict(pack=True), "group": dict(group=4), "working_resolution": dict(seg_long_side=LONG),
            "no_flat": dict(flat=None)}


def make_page(net=True):
    """noisy bright paper and four dark blocks: one on a disc of one colour; one on a disc with a colour ramp (alone in its tile core, in
    sight -- halo 8 -- of the tile to its right); one directly on the noise, across four tile cores; one on a ramp disc that a one-pixel
    line 30 grey levels darker cuts through.  ``net=False``: the first two only."""
    rng = np.random.default_rng(53)
    page = rng.integers(200, 256, size=(H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    dark = lambda shape: rng.integers(0, 40, size=shape + (3,), dtype=np.uint8)
    page[(yy - 24) ** 2 + (xx - 36) ** 2 <= 22 * 22] = DISC
    page[19:30, 30:45] = dark((11, 15))
    disc = (yy - 120) ** 2 + (xx - 36) ** 2 <= 24 * 24
    ramp = np.stack([100 + 2 * (xx - 12), 150 - (yy - 96), 60 + (xx - 12) + (yy - 96)], axis=-1)
    page[disc] = ramp[disc]
    page[115:126, 30:45] = dark((11, 15))
    if net:
        page[88:105, 88:105] = dark((17, 17))
        disc = (yy - 115) ** 2 + (xx - 160) ** 2 <= 24 * 24
        ramp = np.stack([125 + (xx - 136), 130 + (yy - 91), 140 + 0 * xx], axis=-1)
        page[disc] = ramp[disc]
        page[:, 173][disc[:, 173]] = 95                    # not text for the segmenter, a hard edge for the stage: it crosses the ring, not the block
        page[110:121, 150:171] = dark((11, 21))
    return page


def restatement(dev, page, flat=TOL, long_side=None, hull=False):
    """-> dict: clean, mask (0 / 255), rest (0 / 1), painted, the smooth rows, the flat stage's result, the labelled components"""
    g = tile_grid(H, W, TILE, HALO)
    _, final, exp, area, _ = whole_page(page, long_side, 0, hull=hull, max_regions=MAXR)
    comp = expected(final, 8, 0, g) if hull else exp      # hull pixels carry no label: the filled plane is labelled once more
    mask = final * np.uint8(255)
    ff = None
    painted, rest = page, final
    if flat is not None:
        ff = T.flat_fill_regions(page, mask, flat, ring=RING, max_regions=MAXR, device=dev)
        assert np.array_equal(ff.regions.table, comp["table"])
        painted, rest = ff.painted, ff.rest // 255
    rows = smooth_ref(painted, rest, comp["labels"], comp["table"], comp["n"][1], RING, TOL)
    smooth_px = np.isin(comp["labels"], comp["table"][rows[:, 0] != 0, 0]) & (rest != 0)
    whole = T.harmonic_fill(painted, rest * np.uint8(255), sweeps=8, device=dev)
    painted = np.where(smooth_px[..., None], whole, painted)
    rest = rest * ~smooth_px
    clean = np.where(rest[..., None] > 0, FILL, painted)
    return dict(clean=clean, mask=mask, rest=rest, painted=painted, rows=rows, flat=ff, comp=comp, exp=exp, area=area, smooth_px=smooth_px)


@both_backends
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_smooth_equals_the_restatement(backend, variant, monkeypatch):
    kw = dict(flat=TOL, flat_ring=RING)
    kw.update(VARIANTS[variant])
    page = make_page()
    g = tile_grid(H, W, TILE, HALO)
    with BACKENDS[backend]() as dev:
        ref = restatement(dev, page, kw["flat"], kw.get("seg_long_side"), kw.get("hull", False))
        clean, mask, eraser, fill_calls, copies = spied_run(dev, monkeypatch, page, smooth=TOL, smooth_ring=RING, smooth_sweeps=8, **kw)
    rows, comp = ref["rows"], ref["comp"]
    # the routes: the table holds the blocks in raster order of their first pixels: one colour, noise, cut ramp, ramp
    assert len(rows) == 4
    if kw["flat"] is not None:
        assert ref["flat"].is_flat.tolist() == [True, False, False, False] and rows[:, 0].tolist() == [0, 0, 0, 1], (rows, "flat / net / net / smooth")
        assert rows[0].tolist() == [0, 0, 0, 0, 0], "a painted region has no text left: an empty row"
    else:
        assert rows[:, 0].tolist() == [1, 0, 0, 1], "without the flat stage the one-colour disc is smooth as well"
    assert rows[2, 0] == 0 and rows[2, 1:4].max() >= 25 and rows[3, 1:4].max() <= 2, "the line trips the cut disc, the ramp passes"
    # exactly one synchronisation before the filler: [core counts | found, kept | table | flat rows | smooth rows] (+ what rides with it)
    words = g.count + 2 + (16 if kw["flat"] is not None else 11) * MAXR
    words += {"hull": g.count + 2 + 7 * MAXR, "group": MAXR + 1}.get(variant, 0)
    assert copies == [(torch.int32, words)], copies
    assert np.array_equal(mask, ref["mask"]), int((mask != ref["mask"]).sum())
    assert np.array_equal(clean, ref["clean"]), int((clean != ref["clean"]).sum())
    assert np.array_equal(clean[mask == 0], page[mask == 0])
    labels = comp["labels"]
    one_colour, noise, cut, ramp = (labels == comp["table"][k][0] for k in range(4))
    assert one_colour[19:30, 30:45].all() and ramp[115:126, 30:45].all() and noise[88:105, 88:105].all() and cut[110:121, 150:171].all()
    assert all(mask[m].all() for m in (one_colour, noise, cut, ramp)), "the mask holds every region"
    assert bool((clean[noise] == FILL).all()) and bool((clean[cut] == FILL).all()) and bool((clean[ramp] != FILL).any(axis=-1).all())
    if kw["flat"] is not None:
        assert bool((clean[one_colour] == DISC).all())
    want = np.stack([100 + 2 * (np.nonzero(ramp)[1] - 12), 150 - (np.nonzero(ramp)[0] - 96), 60 + (np.nonzero(ramp)[1] - 12) + (np.nonzero(ramp)[0] - 96)], axis=-1)
    assert int(np.abs(clean[ramp].astype(int) - want).max()) <= 2, "the ramp goes on under the block"
    # the filler saw holes on the two net blocks only, the painted and the filled block as valid pixels, and never the smooth block's tile
    after = core_counts(ref["rest"], g)
    selected = [t for t in range(g.count) if after[t] > 0]
    assert core_counts(ref["mask"] // 255, g)[SMOOTH_TILE] > 0 and SMOOTH_TILE not in selected and NEIGHBOUR_TILE in selected and len(selected) == 5
    imgs, planes = np.concatenate([c[0] for c in fill_calls]), np.concatenate([c[1] for c in fill_calls])
    stats = eraser.last_stats
    if variant == "pack":
        origins, rects = T.plan_fill_windows(comp["table"][1:3, 2:6], H, W, TILE, HALO)
        assert len(origins) == 2 and stats["packed"] and stats["windows"] == 2 and stats["grid_selected"] == 5
        want_imgs, want_planes = ref_windows_fill(ref["painted"], ref["rest"], TILE, origins)
    else:
        want_imgs, want_planes = fill_tiles(ref["painted"], ref["rest"], g, selected)
        assert stats["selected"] == 5
        k = selected.index(NEIGHBOUR_TILE)                 # the tile to the right of the smooth block sees it in its halo, as valid pixels
        oy, ox = g.origin(NEIGHBOUR_TILE)
        ys, xs = np.nonzero(ramp[oy:oy + TILE, ox:ox + TILE])
        assert len(ys) > 0 and bool((planes[k][ys, xs] == 1).all())
        assert np.array_equal(imgs[k][ys, xs], ref["painted"][ys + oy, xs + ox].astype(np.float32) / np.float32(255.0))
    assert np.array_equal(planes, want_planes) and np.array_equal(imgs, want_imgs)
    # statistics and regions
    flat_px = int(one_colour.sum()) if kw["flat"] is not None else 0
    smooth_px = int(ref["smooth_px"].sum())
    assert smooth_px == int(ramp.sum()) + (0 if kw["flat"] is not None else int(one_colour.sum()))
    assert stats["smooth_regions"] == int(rows[:, 0].sum()) and stats["smooth_pixels"] == smooth_px
    assert stats["text_pixels"] == int(mask.sum()) // 255 and stats["tiles"] == g.count
    if kw["flat"] is not None:
        assert stats["flat_regions"] == 1 and stats["flat_pixels"] == flat_px
    else:
        assert "flat_regions" not in stats and "flat" not in eraser.last_regions
    reg = eraser.last_regions
    assert sorted(reg["smooth"]) == ["is_smooth", "ring_pixels", "step", "table"]
    assert np.array_equal(reg["smooth"]["table"], comp["table"]) and np.array_equal(reg["smooth"]["is_smooth"], rows[:, 0] != 0)
    assert reg["smooth"]["step"].dtype == np.uint8 and np.array_equal(reg["smooth"]["step"], rows[:, 1:4])
    assert np.array_equal(reg["smooth"]["ring_pixels"], rows[:, 4])
    assert np.array_equal(reg["table"], ref["exp"]["table"])
    if variant == "hull":
        assert np.array_equal(reg["hull_area"], ref["area"])
    if variant == "group":
        assert reg["members"].tolist() == [1, 1, 1, 1] and stats["blocks"] == 4


@both_backends
def test_a_page_of_flat_and_smooth_text_never_calls_the_filler(backend, monkeypatch):
    page = make_page(net=False)
    with BACKENDS[backend]() as dev:
        ref = restatement(dev, page)
        clean, mask, eraser, fill_calls, copies = spied_run(dev, monkeypatch, page, flat=TOL, flat_ring=RING, smooth=TOL)
        only = T.TextEraser(standin_segmenter, standin_filler, mean=MEAN, std=STD, tile=TILE, halo=HALO, dilate=DILATE, device=dev,
                            smooth=TOL)(torch.from_numpy(page))
        ref_only = restatement(dev, page, flat=None)
    assert ref["flat"].is_flat.tolist() == [True, False] and ref["rows"][:, 0].tolist() == [0, 1] and not ref["rest"].any()
    assert fill_calls == [] and copies == [(torch.int32, 20 + 2 + 16 * MAXR)]
    assert np.array_equal(mask, ref["mask"]) and np.array_equal(clean, ref["clean"]) and mask.any()
    assert np.array_equal(clean[mask == 0], page[mask == 0]) and not (clean[mask > 0] == FILL).all(axis=-1).any()
    n_flat, n_smooth = int(ref["flat"].regions.table[0, 1]), int(ref["smooth_px"].sum())
    assert eraser.last_stats == {"tiles": 20, "selected": 0, "text_pixels": n_flat + n_smooth, "flat_regions": 1, "flat_pixels": n_flat,
                                 "smooth_regions": 1, "smooth_pixels": n_smooth}
    assert isinstance(only[0], torch.Tensor) and np.array_equal(only[0].numpy(), ref_only["clean"]) and np.array_equal(only[1].numpy(), ref["mask"])
    assert ref_only["rows"][:, 0].tolist() == [1, 1]


@both_backends
def test_default_is_the_parents_result(backend, monkeypatch):
    """smooth=None: the outputs of the parent's path, its last_stats keys, and no call of a new entry point"""
    from text_segmentation_image_inpainting_amd import _lib, fill, pipeline, regions
    from tests.test_flat_kernels import flat_ref
    names = []
    real = _lib.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)

    page = make_page()
    clean_ref, final, exp, _, _ = whole_page(page, None, 0)
    painted, rest, _, rows = flat_ref(page, final, exp["labels"], exp["table"], exp["n"][1], RING, TOL)
    with BACKENDS[backend]() as dev:
        for mod in (_lib, pipeline, regions, fill):
            monkeypatch.setattr(mod, "call", spy)
        kw = dict(mean=MEAN, std=STD, tile=TILE, halo=HALO, dilate=DILATE, device=dev)
        default = T.TextEraser(standin_segmenter, standin_filler, **kw)
        clean, mask = default(page)
        flat_only = T.TextEraser(standin_segmenter, standin_filler, flat=TOL, flat_ring=RING, max_regions=MAXR, **kw)
        clean_f, mask_f = flat_only(page)
        assert not [n for n in names if n.startswith("tsii_smooth") or n == "tsii_harmonic_fill"] and default.smooth is None
        T.TextEraser(standin_segmenter, standin_filler, flat=TOL, smooth=TOL, **kw)(page)
        at = names.index("tsii_smooth_regions_classify")
        assert names[at - 1:at + 3] == ["tsii_flat_regions", "tsii_smooth_regions_classify", "tsii_harmonic_fill", "tsii_smooth_regions_apply"]
        assert names.count("tsii_smooth_regions_classify") == names.count("tsii_smooth_regions_apply") == names.count("tsii_harmonic_fill") == 1
    assert np.array_equal(mask, final * 255) and np.array_equal(clean, clean_ref)
    assert np.array_equal(mask_f, mask) and np.array_equal(clean_f, np.where(rest[..., None] > 0, FILL, painted))
    assert sorted(default.last_stats) == ["selected", "text_pixels", "tiles"] and default.last_regions is None
    assert sorted(flat_only.last_stats) == ["flat_pixels", "flat_regions", "selected", "text_pixels", "tiles"]
    assert sorted(flat_only.last_regions) == ["flat", "found", "kept", "table", "truncated"]


def test_arguments_are_checked():
    for kw in (dict(smooth=-1), dict(smooth=256), dict(smooth=1.5), dict(smooth=True), dict(smooth=8, smooth_ring=0), dict(smooth=8, smooth_ring=9),
               dict(smooth_ring=0), dict(smooth=8, smooth_sweeps=17), dict(smooth=8, smooth_sweeps=-1), dict(smooth_sweeps=2.5)):
        with pytest.raises(ValueError, match="smooth"):
            T.TextEraser(standin_segmenter, standin_filler, device="cpu", **kw)
    eraser = T.TextEraser(standin_segmenter, standin_filler, device="cpu", smooth=0)
    assert eraser.regions and (eraser.smooth, eraser.smooth_ring, eraser.smooth_sweeps) == (0, 3, 8) and eraser.flat is None
