"""``TextEraser(tone=T)``: text regions whose surroundings are a periodic pattern are filled from one period away on the device and never
reach the filler; the route order is flat, then smooth, then tone, then the net.

Stand-in nets for which tiling cannot matter (the per-pixel segmenter and the constant-colour filler of
``tests/test_text_eraser_working_resolution.py``), so the tiled run must be EQUAL to a whole-page restatement: ``whole_page`` of
``tests/test_text_eraser_hull.py`` up to the final text plane, ``flat_fill_regions`` on it, ``smooth_fill_regions`` on what is left, the
tone decision of ``tests/test_tone_kernels.py`` (per region: dilation, minus the text, whole-array shifted differences, a Python walk) on
what is left of that, then the filler's colour on the rest.  Every case runs on the emulator (CPU suite) and, with -m gpu, on the chip.
"""
import numpy as np
import pytest
import torch

import text_segmentation_image_inpainting_amd as T
from tests.backends import BACKENDS, both_backends
from tests.test_fill_windows_kernels import ref_windows_fill
from tests.test_text_eraser import MEAN, STD, core_counts, fill_tiles, to_byte
from tests.test_text_eraser_flat import spied_run
from tests.test_text_eraser_hull import whole_page
from tests.test_text_eraser_working_resolution import COLOUR, DILATE, HALO, LONG, TILE, standin_filler, standin_segmenter
from tests.test_text_regions import expected
from tests.test_tone_kernels import tone_ref
from text_segmentation_image_inpainting_amd.pipeline import tile_grid

H, W = 150, 217                                           # 4 x 5 tiles with cores of 48 pixels
TOL, RING, MAXR = 8, 3, 32
TONE_RING, PERIOD = 6, 4                                  # the lattice's vertical vector (5, 0) is out of reach: nothing maps the cutting line to itself
DISC = (90, 160, 230)
DOT, GROUND = (240, 150, 180), (170, 190, 210)
FILL = to_byte(np.asarray(COLOUR, np.float32))
TONE_TILE = 3                                             # the core (0..48, 144..192) holds the tone block and nothing else
ROUTES = dict(flat=TOL, flat_ring=RING, smooth=TOL, smooth_ring=RING, smooth_sweeps=8)
VARIANTS = {"plain": {}, "hull": dict(hull=True), "pack": dict(pack=True), "group": dict(group=4), "working_resolution": dict(seg_long_side=LONG),
            "no_flat": dict(flat=None), "no_smooth": dict(smooth=None), "tone_only": dict(flat=None, smooth=None)}


def lattice(yy, xx):
    return np.where(((3 * yy + xx) % 5 == 0)[..., None], np.array(DOT), np.array(GROUND)).astype(np.uint8)


def make_page(net=True):
    """noisy bright paper and five dark blocks: one on a disc of one colour; one on a disc with a colour ramp; one on a disc of a dot
    lattice (alone in its tile core); one directly on the noise, across four tile cores; one on a lattice disc that a one-pixel dark line
    cuts through.  ``net=False``: the first three only."""
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
    disc = (yy - 24) ** 2 + (xx - 162) ** 2 <= 24 * 24
    page[disc] = lattice(yy, xx)[disc]
    page[19:30, 155:170] = dark((11, 15))
    if net:
        page[88:105, 88:105] = dark((17, 17))
        disc = (yy - 115) ** 2 + (xx - 162) ** 2 <= 24 * 24
        page[disc] = lattice(yy, xx)[disc]
        page[:, 175][disc[:, 175]] = 95                    # not text for the segmenter, an outlier for the stage: it crosses the ring, not the block
        page[110:121, 152:171] = dark((11, 19))
    return page


def restatement(dev, page, flat=TOL, smooth=TOL, long_side=None, hull=False):
    """-> dict: clean, mask (0 / 255), rest (0 / 1), painted, the tone rows, the flat and smooth stages' results, the labelled components"""
    g = tile_grid(H, W, TILE, HALO)
    _, final, exp, area, _ = whole_page(page, long_side, 0, hull=hull, max_regions=MAXR)
    comp = expected(final, 8, 0, g) if hull else exp      # hull pixels carry no label: the filled plane is labelled once more
    mask = final * np.uint8(255)
    ff = sf = None
    painted, rest = page, final
    if flat is not None:
        ff = T.flat_fill_regions(painted, mask, flat, ring=RING, max_regions=MAXR, device=dev)
        painted, rest = ff.painted, ff.rest // 255
    if smooth is not None:
        sf = T.smooth_fill_regions(painted, rest * np.uint8(255), smooth, ring=RING, sweeps=8, max_regions=MAXR, device=dev)
        painted, rest = sf.painted, sf.text // 255
    before = rest
    rows, painted, rest, _ = tone_ref(painted, rest, comp["labels"], comp["table"], comp["n"][1], TONE_RING, PERIOD, TOL)
    clean = np.where(rest[..., None] > 0, FILL, painted)
    return dict(clean=clean, mask=mask, rest=rest, painted=painted, rows=rows, flat=ff, smooth=sf, comp=comp, exp=exp, area=area,
                tone_px=(before != 0) & (rest == 0))


@both_backends
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_tone_equals_the_restatement(backend, variant, monkeypatch):
    kw = dict(ROUTES)
    kw.update(VARIANTS[variant])
    page = make_page()
    g = tile_grid(H, W, TILE, HALO)
    with BACKENDS[backend]() as dev:
        ref = restatement(dev, page, kw["flat"], kw["smooth"], kw.get("seg_long_side"), kw.get("hull", False))
        clean, mask, eraser, fill_calls, copies = spied_run(dev, monkeypatch, page, tone=TOL, tone_ring=TONE_RING, tone_period=PERIOD, **kw)
    rows, comp = ref["rows"], ref["comp"]
    # the routes: the table holds the blocks in raster order of their first pixels: one colour, lattice, noise, cut lattice, ramp
    assert len(rows) == 5 and rows[:, 0].tolist() == [0, 1, 0, 0, 0], (rows, "flat / tone / net / net / smooth")
    assert rows[1].tolist()[:4] in ([1, 1, 2, 0], [1, 2, -1, 0]) and rows[1][5] > TOL, "one of the lattice's two shortest vectors, no error"
    assert rows[2].tolist()[:4] == [0, 0, 0, 0] and rows[3].tolist()[:4] == [0, 0, 0, 0], "noise and the cut lattice have no candidate"
    if kw["flat"] is not None:
        assert ref["flat"].is_flat.tolist() == [True, False, False, False, False] and rows[0].tolist() == [0] * 6, "a painted region: an empty row"
    if kw["smooth"] is not None:
        assert rows[4].tolist() == [0] * 6, "a filled region: an empty row"
    else:
        assert rows[4][4] > 0 and rows[4][5] <= TOL, "the ramp is not textured"
    if kw["flat"] is None and kw["smooth"] is None:
        assert rows[0][4] > 0 and rows[0][5] == 0, "one colour is not textured"
    # exactly one synchronisation before the filler: [core counts | found, kept | table | flat rows | smooth rows | tone rows] (+ what rides with it)
    words = g.count + 2 + (12 + 5 * (kw["flat"] is not None) + 5 * (kw["smooth"] is not None)) * MAXR
    words += {"hull": g.count + 2 + 7 * MAXR, "group": MAXR + 1}.get(variant, 0)
    assert copies == [(torch.int32, words)], copies
    assert np.array_equal(mask, ref["mask"]), int((mask != ref["mask"]).sum())
    assert np.array_equal(clean, ref["clean"]), int((clean != ref["clean"]).sum())
    assert np.array_equal(clean[mask == 0], page[mask == 0])
    labels = comp["labels"]
    one_colour, tone, noise, cut, ramp = (labels == comp["table"][k][0] for k in range(5))
    assert one_colour[19:30, 30:45].all() and tone[19:30, 155:170].all() and noise[88:105, 88:105].all() and cut[110:121, 152:171].all()
    assert ramp[115:126, 30:45].all() and all(mask[m].all() for m in (one_colour, tone, noise, cut, ramp)), "the mask holds every region"
    assert bool((clean[noise] == FILL).all()) and bool((clean[cut] == FILL).all())
    yy, xx = np.mgrid[0:H, 0:W]
    assert np.array_equal(clean[tone], lattice(yy, xx)[tone]), "the lattice goes on under the block, byte for byte"
    # the filler saw holes on the net blocks only and never the tone block's tile
    after = core_counts(ref["rest"], g)
    selected = [t for t in range(g.count) if after[t] > 0]
    n_net = 2 + (kw["flat"] is None and kw["smooth"] is None) + (kw["smooth"] is None)
    assert core_counts(ref["mask"] // 255, g)[TONE_TILE] > 0 and TONE_TILE not in selected and len(selected) == 3 + n_net
    imgs, planes = np.concatenate([c[0] for c in fill_calls]), np.concatenate([c[1] for c in fill_calls])
    stats = eraser.last_stats
    if variant == "pack":
        origins, rects = T.plan_fill_windows(comp["table"][2:4, 2:6], H, W, TILE, HALO)
        assert len(origins) == 2 and stats["packed"] and stats["windows"] == 2 and stats["grid_selected"] == 5
        want_imgs, want_planes = ref_windows_fill(ref["painted"], ref["rest"], TILE, origins)
    else:
        want_imgs, want_planes = fill_tiles(ref["painted"], ref["rest"], g, selected)
        assert stats["selected"] == len(selected)
    assert np.array_equal(planes, want_planes) and np.array_equal(imgs, want_imgs)
    # statistics and regions
    tone_px = int(ref["tone_px"].sum())
    assert tone_px == int(tone.sum()) and stats["tone_regions"] == 1 and stats["tone_pixels"] == tone_px
    assert stats["text_pixels"] == int(mask.sum()) // 255 and stats["tiles"] == g.count
    assert ("flat_regions" in stats) == (kw["flat"] is not None) and ("smooth_regions" in stats) == (kw["smooth"] is not None)
    reg = eraser.last_regions
    assert sorted(reg["tone"]) == ["err", "is_tone", "ring_pixels", "shift", "step", "table"]
    assert np.array_equal(reg["tone"]["table"], comp["table"]) and np.array_equal(reg["tone"]["is_tone"], rows[:, 0] != 0)
    assert np.array_equal(reg["tone"]["shift"], rows[:, 1:3]) and np.array_equal(reg["tone"]["err"], rows[:, 3])
    assert np.array_equal(reg["tone"]["ring_pixels"], rows[:, 4]) and np.array_equal(reg["tone"]["step"], rows[:, 5])
    assert np.array_equal(reg["table"], ref["exp"]["table"])
    if variant == "hull":
        assert np.array_equal(reg["hull_area"], ref["area"])
    if variant == "group":
        assert reg["members"].tolist() == [1] * 5 and stats["blocks"] == 5


@both_backends
def test_a_page_of_flat_smooth_and_tone_text_never_calls_the_filler(backend, monkeypatch):
    page = make_page(net=False)
    with BACKENDS[backend]() as dev:
        ref = restatement(dev, page)
        clean, mask, eraser, fill_calls, copies = spied_run(dev, monkeypatch, page, tone=TOL, tone_ring=TONE_RING, tone_period=PERIOD, **ROUTES)
    assert ref["rows"][:, 0].tolist() == [0, 1, 0] and not ref["rest"].any()
    assert fill_calls == [] and copies == [(torch.int32, 20 + 2 + 22 * MAXR)]
    assert np.array_equal(mask, ref["mask"]) and np.array_equal(clean, ref["clean"]) and mask.any()
    assert np.array_equal(clean[mask == 0], page[mask == 0]) and not (clean[mask > 0] == FILL).all(axis=-1).any()
    stats = eraser.last_stats
    assert stats["selected"] == 0 and stats["flat_regions"] == stats["smooth_regions"] == stats["tone_regions"] == 1
    assert stats["text_pixels"] == stats["flat_pixels"] + stats["smooth_pixels"] + stats["tone_pixels"] == int(mask.sum()) // 255


@both_backends
def test_default_is_the_parents_result(backend, monkeypatch):
    """tone=None: the outputs of the parent's path, its last_stats keys, and no call of the new entry points"""
    from text_segmentation_image_inpainting_amd import _lib, fill, pipeline, regions
    names = []
    real = _lib.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)

    page = make_page()
    clean_ref = whole_page(page, None, 0)[0]
    with BACKENDS[backend]() as dev:
        for mod in (_lib, pipeline, regions, fill):
            monkeypatch.setattr(mod, "call", spy)
        kw = dict(mean=MEAN, std=STD, tile=TILE, halo=HALO, dilate=DILATE, device=dev)
        default = T.TextEraser(standin_segmenter, standin_filler, **kw)
        clean, mask = default(page)
        routed = T.TextEraser(standin_segmenter, standin_filler, max_regions=MAXR, **ROUTES, **kw)
        routed(page)
        assert not [n for n in names if n.startswith("tsii_tone")] and default.tone is None and routed.tone is None
        T.TextEraser(standin_segmenter, standin_filler, tone=TOL, **ROUTES, **kw)(page)
        at = names.index("tsii_tone_regions")
        assert names[at - 1] == "tsii_smooth_regions_apply" and names.count("tsii_tone_regions") == 1
    assert np.array_equal(clean, clean_ref)
    assert sorted(default.last_stats) == ["selected", "text_pixels", "tiles"] and default.last_regions is None
    assert sorted(routed.last_stats) == ["flat_pixels", "flat_regions", "selected", "smooth_pixels", "smooth_regions", "text_pixels", "tiles"]
    assert sorted(routed.last_regions) == ["flat", "found", "kept", "smooth", "table", "truncated"]


def test_arguments_are_checked():
    for kw in (dict(tone=-1), dict(tone=256), dict(tone=1.5), dict(tone=True), dict(tone=8, tone_ring=0), dict(tone=8, tone_ring=17),
               dict(tone_ring=0), dict(tone=8, tone_period=1), dict(tone=8, tone_period=17), dict(tone_period=2.5)):
        with pytest.raises(ValueError, match="tone"):
            T.TextEraser(standin_segmenter, standin_filler, device="cpu", **kw)
    eraser = T.TextEraser(standin_segmenter, standin_filler, device="cpu", tone=0)
    assert eraser.regions and (eraser.tone, eraser.tone_ring, eraser.tone_period) == (0, 8, 12) and eraser.flat is None and eraser.smooth is None
