"""``TextEraser(seg_long_side=...)``: the segmenter at a working resolution, both resamplings on the device.

Stand-in nets for which tiling cannot matter -- a per-pixel segmenter and a constant-colour filler -- so the tiled run must be EQUAL to
a whole-page numpy restatement: Pillow resize -> normalise -> stand-in -> threshold -> 3 x 3 dilation -> integer up-sample (-> regions)
-> compose.  Call spies pin that the segmenter saw the working grid's tiles and the filler only page-grid tiles with text.  Every case
runs on the emulator (CPU suite) and, with -m gpu, on the chip.
"""
import numpy as np
import pytest
import torch
from PIL import Image

import text_segmentation_image_inpainting_amd as T
from tests.backends import BACKENDS, both_backends
from tests.test_resample_kernels import ref_plane_up
from tests.test_text_eraser import MEAN, STD, core_counts, dilate_np, fill_tiles, normalise, seg_tiles, to_byte
from tests.test_text_regions import expected
from text_segmentation_image_inpainting_amd import _lib
from text_segmentation_image_inpainting_amd.pipeline import tile_grid

TILE, HALO, DILATE = 64, 8, 3
H, W, LONG = 150, 217, 96                                 # working size 64 x 96: 2 x 2 tiles for the segmenter, 4 x 5 on the page
COLOUR = (0.25, 0.5, 0.75)
NEW_NAMES = {"tsii_page_resize_u8", "tsii_text_plane_up", "tsii_resize_coeffs_u8", "tsii_resize_taps"}


def standin_segmenter(x):
    """per pixel: dark ink -> positive logit"""
    return -(x[:, 0:1] * 0.5 + x[:, 1:2] * 0.25 + x[:, 2:3] * 0.25 + 0.4)


def standin_filler(args):
    x, _ = args
    return torch.tensor(COLOUR, dtype=torch.float32, device=x.device).view(1, 3, 1, 1).expand(x.shape[0], 3, x.shape[2], x.shape[3])


def make_page(h, w, seed, small_blob=False):
    """bright paper, one dark blob across several page tiles and (``small_blob``) a speck alone in the bottom right corner"""
    rng = np.random.default_rng(seed)
    page = rng.integers(200, 256, size=(h, w, 3), dtype=np.uint8)
    page[30:70, 40:110] = rng.integers(0, 40, size=(40, 70, 3), dtype=np.uint8)
    if small_blob:
        page[h - 14:h - 7, w - 16:w - 9] = rng.integers(0, 40, size=(7, 7, 3), dtype=np.uint8)
    return page


def whole_page(page, long_side, min_area=0):
    """the restatement -> (clean, text plane on the page, working page, text plane before the region filter)"""
    h, w = page.shape[:2]
    g = tile_grid(h, w, TILE, HALO)
    hs, ws = T.working_size(h, w, long_side)
    small = page if (hs, ws) == (h, w) else np.asarray(Image.fromarray(page).resize((ws, hs), Image.BICUBIC))
    logits = standin_segmenter(torch.from_numpy(normalise(small)).permute(2, 0, 1)[None])[0, 0].numpy()
    text_s = dilate_np(logits > np.float32(0.0), DILATE)
    text = text_s if (hs, ws) == (h, w) else ref_plane_up(text_s, g)[0]
    unfiltered = text
    if min_area > 1:
        text = expected(text, 8, min_area, g)["text"]
    clean = np.where(text[..., None] > 0, to_byte(np.asarray(COLOUR, np.float32)), page)
    return clean, text, small, unfiltered


@both_backends
def test_working_resolution_equals_the_restatement(backend):
    page = make_page(H, W, seed=31)
    g = tile_grid(H, W, TILE, HALO)
    hs, ws = T.working_size(H, W, LONG)
    assert (hs, ws) == (64, 96)
    gs = tile_grid(hs, ws, TILE, HALO)
    clean_ref, text_ref, small, _ = whole_page(page, LONG)
    seg_calls, fill_calls = [], []

    def seg_spy(x):
        seg_calls.append(x.detach().cpu().permute(0, 2, 3, 1).numpy().copy())
        return standin_segmenter(x)

    def fill_spy(args):
        fill_calls.append(args[1].parts[0].plane.detach().cpu().numpy().copy())
        return standin_filler(args)

    with BACKENDS[backend]() as dev:
        eraser = T.TextEraser(seg_spy, fill_spy, mean=MEAN, std=STD, tile=TILE, halo=HALO, dilate=DILATE, tile_batch=3, device=dev,
                              seg_long_side=LONG)
        clean, mask = eraser(page)
        clean_t, mask_t = eraser(torch.from_numpy(page))
    assert np.array_equal(mask, text_ref * 255), int((mask != text_ref * 255).sum())
    assert np.array_equal(clean, clean_ref), int((clean != clean_ref).sum())
    assert np.array_equal(clean[mask == 0], page[mask == 0]) and bool((clean != page).any())
    assert isinstance(clean_t, torch.Tensor) and np.array_equal(clean_t.numpy(), clean) and np.array_equal(mask_t.numpy(), mask)
    # the segmenter saw the working page's tiles (4, in batches of 3), the filler exactly the page-grid tiles with text
    n_seg = len(seg_calls) // 2
    assert [len(c) for c in seg_calls[:n_seg]] == [3, 1] and gs.count == 4
    assert np.array_equal(np.concatenate(seg_calls[:n_seg]), seg_tiles(small, gs))
    counts = core_counts(text_ref, g)
    selected = [t for t in range(g.count) if counts[t] > 0]
    assert 1 < len(selected) < g.count == 20
    _, planes = fill_tiles(page, text_ref, g, selected)
    assert np.array_equal(np.concatenate(fill_calls[:len(fill_calls) // 2]), planes)
    assert eraser.last_stats == {"tiles": 20, "selected": len(selected), "text_pixels": int(text_ref.sum()), "seg_tiles": 4, "seg_size": (64, 96)}


@both_backends
def test_min_area_is_measured_on_the_page(backend):
    """the speck is 4 x 4 working pixels after the dilation and about 10 x 10 on the page: a ``min_area`` between the two keeps it only
    if regions are measured at page resolution; one above its page area drops it"""
    page = make_page(H, W, seed=32, small_blob=True)
    g = tile_grid(H, W, TILE, HALO)
    _, _, _, unfiltered = whole_page(page, LONG)
    areas = sorted(expected(unfiltered, 8, 0, g)["table"][:, 1])
    assert len(areas) == 2 and 36 < areas[0] < areas[1], areas
    results = {}
    with BACKENDS[backend]() as dev:
        for min_area in (36, areas[0] + 1):
            eraser = T.TextEraser(standin_segmenter, standin_filler, mean=MEAN, std=STD, tile=TILE, halo=HALO, dilate=DILATE, device=dev,
                                  seg_long_side=LONG, min_area=min_area)
            results[min_area] = eraser(page) + (eraser.last_regions, eraser.last_stats)
    for min_area, kept in ((36, 2), (areas[0] + 1, 1)):
        clean, mask, regions, stats = results[min_area]
        clean_ref, text_ref, _, _ = whole_page(page, LONG, min_area)
        assert (regions["found"], regions["kept"]) == (2, kept)
        assert np.array_equal(regions["table"], expected(unfiltered, 8, min_area, g)["table"])
        assert np.array_equal(mask, text_ref * 255) and np.array_equal(clean, clean_ref)
        assert stats["text_pixels"] == int(text_ref.sum()) and stats["seg_tiles"] == 4
    assert not results[areas[0] + 1][1][H - 30:, W - 30:].any() and results[36][1][H - 30:, W - 30:].any()


@both_backends
def test_long_side_of_the_page_is_the_default_path(backend, monkeypatch):
    """working size == page size: nothing is resized and the result is the default path's; and with ``seg_long_side=None`` none of the
    new entry points is called and ``last_stats`` keeps its three keys"""
    from text_segmentation_image_inpainting_amd import pipeline
    h, w = 152, 216
    assert T.working_size(h, w, 216) == (h, w)
    page = make_page(h, w, seed=33)
    names = []
    real = _lib.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)

    with BACKENDS[backend]() as dev:
        for mod in (_lib, pipeline):
            monkeypatch.setattr(mod, "call", spy)
        kw = dict(mean=MEAN, std=STD, tile=TILE, halo=HALO, dilate=DILATE, device=dev)
        default = T.TextEraser(standin_segmenter, standin_filler, **kw)
        clean_d, mask_d = default(page)
        assert "tsii_tiles_text_mask" in names and not NEW_NAMES & set(names), names
        assert default.last_stats is not None and sorted(default.last_stats) == ["selected", "text_pixels", "tiles"]
        same = T.TextEraser(standin_segmenter, standin_filler, seg_long_side=216, **kw)
        clean_s, mask_s = same(page)
        assert not NEW_NAMES & set(names), names
        smaller = T.TextEraser(standin_segmenter, standin_filler, seg_long_side=LONG, **kw)
        smaller(page)
        assert {"tsii_page_resize_u8", "tsii_text_plane_up"} <= set(names)
    assert mask_d.any() and np.array_equal(clean_s, clean_d) and np.array_equal(mask_s, mask_d)
    assert same.last_stats == dict(default.last_stats, seg_tiles=default.last_stats["tiles"], seg_size=(h, w))
    clean_ref, text_ref, _, _ = whole_page(page, 216)
    assert np.array_equal(mask_d, text_ref * 255) and np.array_equal(clean_d, clean_ref)


@both_backends
def test_refusals(backend):
    for bad in (100, 0, -8, 12.5):
        with pytest.raises(ValueError, match="multiple of 8"):
            T.TextEraser(standin_segmenter, standin_filler, device="cpu", seg_long_side=bad)
    with BACKENDS[backend]() as dev:
        eraser = T.TextEraser(standin_segmenter, standin_filler, tile=TILE, halo=HALO, device=dev, seg_long_side=8)
        with pytest.raises(ValueError, match="within 8 x"):
            eraser(np.full((100, 70, 3), 255, np.uint8))                 # 100 x 70 -> 8 x 8: more than 8 x per side
        clean, mask = eraser(np.full((64, 40, 3), 255, np.uint8))       # 64 x 40 -> 8 x 8: exactly 8 x, a blank page
        assert eraser.last_stats["seg_size"] == (8, 8) and not mask.any() and bool((clean == 255).all())
