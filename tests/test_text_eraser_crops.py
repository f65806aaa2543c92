"""``TextEraser(crops=(ch, cw))``: rectified crops of every kept table row, cut out of the RAW page on the device behind the geometry stage,
the slots left on the device, their ``info`` riding the page's one read-back.

The stand-in nets and the page of tests/test_text_eraser_geometry.py.  What the stage must give is defined by what it runs on:
``last_crops`` and ``last_regions["crops"]`` have to EQUAL the restatement of tests/test_region_crops.py taken of the raw page and the page's
final ``rect`` (whose own correctness tests/test_text_eraser_geometry.py holds) -- and nothing else may move: the same bytes, stats and other
regions' keys as with ``geometry=True`` alone.  Every case runs on the emulator (CPU suite) and, with -m gpu, on the chip.
"""
import numpy as np
import pytest
import torch

import text_segmentation_image_inpainting_amd as T
from tests.backends import BACKENDS, both_backends
from tests.test_eraser_stage_marks import same
from tests.test_region_crops import header, sample
from tests.test_text_eraser import MEAN, STD
from tests.test_text_eraser_flat import MAXR, spied_run
from tests.test_text_eraser_geometry import H, SEED, W, make_page
from tests.test_text_eraser_working_resolution import DILATE, HALO, LONG, TILE, standin_filler, standin_segmenter
from text_segmentation_image_inpainting_amd import _lib
from text_segmentation_image_inpainting_amd.pipeline import STAGE_MARKS, tile_grid
from text_segmentation_image_inpainting_amd.regions import ReadBack

SIZE, SLOTS = (16, 40), 3                                 # fewer slots than the plain page has rows: the fourth row gets no crop
CONFIGS = {"alone": {}, "group": dict(group=6), "seed": dict(seed=SEED), "working_resolution": dict(seg_long_side=LONG)}


def check_crops(eraser, page, size, slots, orient=0, fill=255, max_ss=4):
    """last_crops and last_regions["crops"] against the restatement on the raw page and the rect the page ended with -> rows served"""
    reg = eraser.last_regions
    n = min(len(reg["rect"]), slots)
    rc = reg["crops"]
    assert isinstance(rc, T.RegionCrops) and rc.info.dtype == np.int32 and rc.info.shape == (n, 10) and eraser.last_stats["crops"] == n
    assert isinstance(eraser.last_crops, torch.Tensor) and eraser.last_crops.dtype == torch.uint8 and tuple(eraser.last_crops.shape) == (slots, *size, 3)
    slots_h = eraser.last_crops.cpu().numpy()
    assert tuple(rc.crops.shape) == (n, *size, 3) and np.array_equal(rc.crops.cpu().numpy(), slots_h[:n])
    assert bool((slots_h[n:] == fill).all()), "slots behind the rows served hold the fill"
    for r in range(n):
        info = header(reg["rect"][r], *size, orient, max_ss)
        assert tuple(int(v) for v in rc.info[r]) == info and info[0] > 0
        want = np.full((*size, 3), fill, np.uint8)
        want[:info[0], :info[1]] = sample(page, info)
        assert np.array_equal(slots_h[r], want), r
    return n


@both_backends
@pytest.mark.parametrize("config", list(CONFIGS))
def test_crops_equal_the_restatement_and_nothing_else_moves(backend, config, monkeypatch):
    kw = CONFIGS[config]
    page = make_page()
    with BACKENDS[backend]() as dev:
        clean, mask, eraser, _, copies = spied_run(dev, monkeypatch, page, crops=SIZE, max_crops=SLOTS, **kw)
        assert eraser.geometry and eraser.regions
        n = check_crops(eraser, page, SIZE, SLOTS)
        crop_h = [eraser.last_regions["crops"].crop(r).cpu().numpy() for r in range(n)]
        clean_p, mask_p, plain, _, copies_p = spied_run(dev, monkeypatch, page, geometry=True, **kw)
        assert plain.last_crops is None
    rows = {"alone": 4, "group": 3, "seed": 3, "working_resolution": None}[config]
    assert rows is None or (len(eraser.last_regions["rect"]) == rows and n == min(rows, SLOTS)), "bar, L, speck and grey blob; see test_text_eraser_geometry"
    # one int32 copy before the filler, larger by exactly 10 words per slot
    assert len(copies) == 1 and len(copies_p) == 1 and copies[0][0] == torch.int32 and copies[0][1] == copies_p[0][1] + 10 * SLOTS, (copies, copies_p)
    assert np.array_equal(clean, clean_p) and np.array_equal(mask, mask_p) and mask.any()
    assert "crops" in eraser.last_regions and "crops" not in plain.last_regions and "crops" not in plain.last_stats
    assert same({k: v for k, v in eraser.last_regions.items() if k != "crops"}, plain.last_regions)
    assert same({k: v for k, v in eraser.last_stats.items() if k != "crops"}, plain.last_stats)
    # the crops show the RAW page: the ink (0..30) is in them, and it is gone from the same place of the cleaned page
    dark = [int((c.max(axis=-1) <= 40).sum()) for c in crop_h]         # the paper is 200 and more, the grey blob 62 and more
    assert max(dark) >= 20, "the bar is dark ink, several crop pixels wide"
    assert int((clean[mask != 0].max(axis=-1) <= 30).sum()) == 0 and int((page[mask != 0].max(axis=-1) <= 30).sum()) > 500


@both_backends
def test_long_orientation_fill_and_supersampling(backend, monkeypatch):
    page = make_page()
    with BACKENDS[backend]() as dev:
        _, _, eraser, _, _ = spied_run(dev, monkeypatch, page, crops=(9, 31), max_crops=6, crop_orient="long", crop_fill=7, crop_supersample=2)
        n = check_crops(eraser, page, (9, 31), 6, orient=1, fill=7, max_ss=2)
        info = eraser.last_regions["crops"].info
    assert n == 4 and bool((info[:, 1] >= info[:, 0]).all()) and bool((info[:, 3] <= 2).all()) and 2 in info[:, 3]


@both_backends
def test_the_mark_sits_between_tone_and_joined(backend):
    assert STAGE_MARKS.index("tone") + 1 == STAGE_MARKS.index("crops") == STAGE_MARKS.index("joined") - 1 and STAGE_MARKS.count("crops") == 1
    page = make_page()
    with BACKENDS[backend]() as dev:
        make = lambda **kw: T.TextEraser(standin_segmenter, standin_filler, mean=MEAN, std=STD, tile=TILE, halo=HALO, dilate=DILATE, device=dev,
                                         max_regions=MAXR, **kw)
        names, off, alone = [], [], []
        eraser, without, only = make(crops=SIZE, group=6, seed=SEED, hull=True, flat=8), make(geometry=True, group=6, seed=SEED, hull=True, flat=8), make(crops=SIZE)
        eraser._mark, without._mark, only._mark = names.append, off.append, alone.append
        eraser(page)
        without(page)
        only(page)
    at = names.index("crops")
    assert names.count("crops") == 1 and names[at - 1:at + 2] == ["flat", "crops", "joined"] and names.index("geometry") < at
    assert "crops" not in off and [n for n in names if n != "crops"] == off
    assert alone[alone.index("geometry") - 1:alone.index("geometry") + 3] == ["regions", "geometry", "crops", "joined"]


@both_backends
def test_default_eraser_never_calls_the_stage(backend, monkeypatch):
    from text_segmentation_image_inpainting_amd import pipeline, regions
    names = []
    real = _lib.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)

    page = make_page()
    g = tile_grid(H, W, TILE, HALO)
    with BACKENDS[backend]() as dev:
        for mod in (_lib, pipeline, regions):
            monkeypatch.setattr(mod, "call", spy)
        kw = dict(mean=MEAN, std=STD, tile=TILE, halo=HALO, dilate=DILATE, device=dev, max_regions=MAXR)
        for opts in ({}, dict(regions=True), dict(geometry=True, hull=True, group=6, seed=SEED, flat=8)):
            eraser = T.TextEraser(standin_segmenter, standin_filler, **opts, **kw)
            assert eraser.crops is None and eraser._layout(g).crops == 0
            eraser(page)
            assert eraser.last_crops is None and "crops" not in eraser.last_stats and "crops" not in (eraser.last_regions or {})
        assert "tsii_region_geometry" in names and "tsii_region_crops" not in names
        T.TextEraser(standin_segmenter, standin_filler, crops=SIZE, hull=True, **kw)(page)
        assert names.count("tsii_region_crops") == 1 and names.index("tsii_region_crops") > names.index("tsii_region_hulls")
    # the read-back without the flag has the words it had
    nt = g.count
    assert ReadBack(nt, MAXR, regions=False).words == nt and ReadBack(nt, MAXR).words == nt + 2 + 6 * MAXR
    assert ReadBack(nt, MAXR, hull=True, geometry=64).words == nt + 2 + 7 * MAXR + MAXR * (16 + 1 + 128)
    assert ReadBack(nt, MAXR, hull=True, group=True, flat=True, seeds=True).words == 2 * (nt + 2 + 6 * MAXR) + MAXR + 5 * MAXR + MAXR + 1 + MAXR + 2
    assert ReadBack(nt, MAXR, hull=True, geometry=64, crops=0).words == ReadBack(nt, MAXR, hull=True, geometry=64).words
    with_crops = ReadBack(nt, MAXR, hull=True, geometry=64, crops=5)
    assert with_crops.words == ReadBack(nt, MAXR, hull=True, geometry=64).words + 50 and with_crops.crop_words == slice(with_crops.words - 50, with_crops.words)
    assert ReadBack(nt, MAXR, regions=False, geometry=64, crops=5).words == nt


def test_arguments_are_checked():
    make = lambda **kw: T.TextEraser(standin_segmenter, standin_filler, device="cpu", **kw)
    for bad in (dict(crops=(0, 8)), dict(crops=(8, 4097)), dict(crops=8), dict(crops=(8.5, 8)), dict(crops=(8, 8), max_crops=0),
                dict(crops=(4096, 4096), max_crops=43), dict(crops=(8, 8), crop_orient="wide"), dict(crops=(8, 8), crop_fill=256),
                dict(crops=(8, 8), crop_supersample=5), dict(max_crops=0), dict(crop_orient="wide"), dict(crop_fill=-1), dict(crop_supersample=0)):
        with pytest.raises(ValueError):
            make(**bad)
    eraser = make(crops=[8, 24])
    assert eraser.regions and eraser.geometry and eraser.crops == (8, 24) and eraser.max_crops == 64
    assert not make().geometry and make().crops is None
