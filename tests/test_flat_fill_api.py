"""``flat_fill_regions`` (regions.py; ``tsii_flat_regions``, "K13: flat regions"): numpy or torch in, the same kind out, one call; equal
to the restatement of ``tests/test_flat_kernels.py`` on its 150 x 217 page.  Emulator (CPU suite) and, with -m gpu, the chip."""
import numpy as np
import pytest
import torch

import text_segmentation_image_inpainting_amd as T
from tests.backends import BACKENDS, both_backends
from tests.test_flat_kernels import case, regions_of

H, W, RING, TOL = 150, 217, 3, 8


@both_backends
def test_flat_fill_regions_api(backend):
    page, text, _, (painted, rest, _, rows) = case("blocks", H, W, 8, RING, TOL)
    exp = regions_of("blocks", H, W, 8)[2]
    few = case("blocks", H, W, 8, RING, TOL, 3)[3]
    mask = (text != 0).astype(np.uint8) * 255
    keep_mask, keep_page = mask.copy(), page.copy()
    with BACKENDS[backend]() as dev:
        r = T.flat_fill_regions(page, mask, TOL, device=dev)
        p_in, m_in = torch.from_numpy(page).to(dev), torch.from_numpy(mask).to(dev)
        rt = T.flat_fill_regions(p_in, m_in, TOL, ring=RING, connectivity=8, max_regions=3, device=dev)
        assert torch.equal(m_in.cpu(), torch.from_numpy(keep_mask)) and torch.equal(p_in.cpu(), torch.from_numpy(keep_page)), "arguments are not modified"
        for t in (rt.painted, rt.rest, rt.regions.labels):
            assert isinstance(t, torch.Tensor) and t.device == m_in.device
        rt_painted, rt_rest = rt.painted.cpu().numpy(), rt.rest.cpu().numpy()
    assert np.array_equal(mask, keep_mask) and np.array_equal(page, keep_page)
    assert isinstance(r, T.FlatFill) and isinstance(r.regions, T.TextRegions)
    assert all(isinstance(a, np.ndarray) for a in (r.painted, r.rest, r.regions.labels))
    assert r.painted.dtype == np.uint8 and np.array_equal(r.painted, painted)
    assert r.rest.dtype == np.uint8 and np.array_equal(r.rest, rest * 255)
    assert r.is_flat.dtype == np.bool_ and np.array_equal(r.is_flat, rows[:, 0] != 0) and 0 < r.is_flat.sum() < len(rows)
    assert r.colour.dtype == np.uint8 and r.colour.shape == (len(rows), 3) and np.array_equal(r.colour, rows[:, 1:4])
    assert r.ring_pixels.dtype == np.int32 and np.array_equal(r.ring_pixels, rows[:, 4])
    assert np.array_equal(r.regions.labels, exp["labels"]) and np.array_equal(r.regions.table, exp["table"])
    assert (r.regions.found, r.regions.kept, r.regions.truncated) == (exp["n"][0], exp["n"][1], False)
    # three table rows of fifteen: the others stay text
    assert np.array_equal(rt_painted, few[0]) and np.array_equal(rt_rest, few[1] * 255) and rt.regions.truncated
    assert len(rt.is_flat) == 3 and np.array_equal(rt.ring_pixels, few[3][:, 4]) and np.array_equal(rt.regions.table, exp["table"][:3])


def test_arguments_are_checked():
    page, mask = np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.uint8)
    for kw in (dict(tol=-1), dict(tol=256), dict(tol=1.5), dict(tol=8, ring=0), dict(tol=8, ring=9), dict(tol=8, ring=2.5),
               dict(tol=8, connectivity=6), dict(tol=8, min_area=-1), dict(tol=8, max_regions=0)):
        with pytest.raises(ValueError):
            T.flat_fill_regions(page, mask, **kw)
    with pytest.raises(ValueError, match="uint8"):
        T.flat_fill_regions(page, np.zeros((4, 4), np.float32), 8)
    with pytest.raises(ValueError, match="uint8"):
        T.flat_fill_regions(page.astype(np.float32), mask, 8)
    with pytest.raises(ValueError, match="page must be"):
        T.flat_fill_regions(np.zeros((4, 5, 3), np.uint8), mask, 8)
