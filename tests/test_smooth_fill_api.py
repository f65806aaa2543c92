"""``smooth_fill_regions`` (regions.py; ``tsii_smooth_regions_classify`` / ``tsii_smooth_regions_apply`` around ``tsii_harmonic_fill``,
"K16: smooth regions"): the stand-alone form of the smooth stage, against the restatement of ``tests/test_smooth_kernels.py`` and
``harmonic_fill`` itself.  Emulator (CPU suite) and, with -m gpu, the chip."""
import numpy as np
import pytest
import torch

import text_segmentation_image_inpainting_amd as T
from tests.backends import BACKENDS, both_backends
from tests.test_flat_kernels import blocks_pattern
from tests.test_smooth_kernels import quarters_page, smooth_ref
from tests.test_text_eraser import to_byte
from tests.test_text_regions import HALO, TILE, expected
from text_segmentation_image_inpainting_amd.pipeline import tile_grid

H, W = 150, 217
TOL, RING = 8, 3


def ramp_page():
    """the 150 x 217 ramp page of tests/test_harmonic_kernels.py::test_ramp, in bytes"""
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = 0.2 + 0.5 * xx / W + 0.25 * yy / H
    return to_byte(np.stack([ramp, 0.9 - 0.6 * ramp, 0.1 + 0.8 * ramp], axis=-1).astype(np.float32))


@both_backends
def test_quarters_page(backend):
    """numpy in, numpy out; a device tensor in, the same device out; the arguments are not modified; ``painted`` on the smooth regions is
    ``harmonic_fill(page, mask)`` byte for byte and the page elsewhere"""
    page, text = quarters_page(H, W, TOL), blocks_pattern(H, W)
    mask = (text != 0).astype(np.uint8) * 255
    exp = expected(text, 8, 0, tile_grid(H, W, TILE, HALO))
    rows = smooth_ref(page, exp["text"], exp["labels"], exp["table"], exp["n"][1], RING, TOL)
    assert 0 < rows[:, 0].sum() < len(rows) == 15
    keep_page, keep_mask = page.copy(), mask.copy()
    with BACKENDS[backend]() as dev:
        got = T.smooth_fill_regions(page, mask, TOL, device=dev)
        whole = T.harmonic_fill(page, mask, device=dev)
        p_in, m_in = torch.from_numpy(page).to(dev), torch.from_numpy(text).to(dev)               # any non-zero byte is text
        got_t = T.smooth_fill_regions(p_in, m_in, TOL, ring=RING, sweeps=8, device=dev)
        assert isinstance(got_t, T.SmoothFill) and all(isinstance(t, torch.Tensor) and t.device == p_in.device for t in (got_t.painted, got_t.text))
        assert torch.equal(p_in.cpu(), torch.from_numpy(keep_page)) and torch.equal(m_in.cpu(), torch.from_numpy(text)), "arguments are not modified"
        painted_t, text_t = got_t.painted.cpu().numpy(), got_t.text.cpu().numpy()
        rough = T.smooth_fill_regions(page, mask, TOL, sweeps=0, device=dev)
    assert np.array_equal(page, keep_page) and np.array_equal(mask, keep_mask)
    assert isinstance(got.painted, np.ndarray) and got.painted.dtype == np.uint8 and got.painted.shape == (H, W, 3)
    assert isinstance(got.text, np.ndarray) and got.text.dtype == np.uint8 and got.text.shape == (H, W)
    assert np.array_equal(got.painted, painted_t) and np.array_equal(got.text, text_t)
    for res in (got, got_t):
        assert np.array_equal(res.table, exp["table"]) and np.array_equal(res.is_smooth, rows[:, 0] != 0)
        assert res.step.dtype == np.uint8 and np.array_equal(res.step, rows[:, 1:4]) and np.array_equal(res.ring_pixels, rows[:, 4])
    smooth_px = np.isin(exp["labels"], exp["table"][rows[:, 0] != 0, 0])
    assert np.array_equal(got.painted[smooth_px], whole[smooth_px]), "the page-level harmonic fill, byte for byte"
    assert np.array_equal(got.painted[~smooth_px], page[~smooth_px])
    assert np.array_equal(got.text, ((exp["labels"] != 0) & ~smooth_px) * np.uint8(255))
    assert np.array_equal(rough.text, got.text) and bool((rough.painted != got.painted).any())


@both_backends
def test_ramp(backend):
    """a 40 x 120 text rectangle in the 150 x 217 ramp page is smooth at tol 2 and comes back within one grey level of the ramp at 8
    sweeps: the bound of tests/test_harmonic_kernels.py::test_ramp, from the float64 restatement there"""
    page = ramp_page()
    mask = np.zeros((H, W), np.uint8)
    mask[55:95, 50:170] = 255
    inked = page.copy()
    inked[mask > 0] = 10                                   # what the page holds under the text plays no part
    with BACKENDS[backend]() as dev:
        got = T.smooth_fill_regions(inked, mask, 2, device=dev)
        hard = T.smooth_fill_regions(inked, mask, 0, device=dev)
    assert got.is_smooth.tolist() == [True] and int(got.step.max()) <= 1 and got.ring_pixels.tolist() == [46 * 126 - 40 * 120]
    assert not got.text.any() and np.array_equal(got.painted[mask == 0], page[mask == 0])
    off = int(np.abs(got.painted[mask > 0].astype(int) - page[mask > 0].astype(int)).max())
    print(f"painted - ramp: {off} grey levels")
    assert off <= 1
    assert hard.is_smooth.tolist() == [False] and np.array_equal(hard.painted, inked) and np.array_equal(hard.text, mask)


@both_backends
def test_truncated_table(backend):
    """max_regions = 2 of four components: the others stay text"""
    text = np.zeros((40, 50), np.uint8)
    for k in range(4):
        text[5 + 6 * k:9 + 6 * k, 10:20] = 255
    page = np.full((40, 50, 3), 90, np.uint8)
    page[text > 0] = 0
    with BACKENDS[backend]() as dev:
        got = T.smooth_fill_regions(page, text, 0, max_regions=2, device=dev)
        dropped = T.smooth_fill_regions(page, text, 0, min_area=41, device=dev)
    assert len(got.table) == 2 and got.is_smooth.tolist() == [True, True] and got.ring_pixels.tolist() == [110, 100]
    assert not got.text[:17].any() and bool((got.text[17:21, 10:20] == 255).all()) and bool((got.text[23:27, 10:20] == 255).all())
    assert bool((got.painted[:17] == 90).all()) and np.array_equal(got.painted[17:], page[17:])
    assert len(dropped.table) == 0 and not dropped.text.any() and np.array_equal(dropped.painted, page)


def test_arguments_are_checked():
    page, mask = np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.uint8)
    for kw in (dict(tol=-1), dict(tol=256), dict(tol=1.5), dict(tol=True), dict(tol=8, ring=0), dict(tol=8, ring=9), dict(tol=8, sweeps=17),
               dict(tol=8, sweeps=-1), dict(tol=8, sweeps=2.5)):
        with pytest.raises(ValueError, match="smooth"):
            T.smooth_fill_regions(page, mask, **kw)
    with pytest.raises(ValueError):
        T.smooth_fill_regions(page, mask, 8, connectivity=6)
    with pytest.raises(ValueError, match="page"):
        T.smooth_fill_regions(page[:3], mask, 8)
