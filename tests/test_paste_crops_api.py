"""``paste_crops``, ``RegionCrops.paste`` and ``check_paste_args`` (``regions.py``; the kernels: tests/test_region_paste.py, whose restatement this
file uses).  The bytes are compared for equality.  Every kernel case runs on the emulator (CPU suite) and, with -m gpu, on the chip.
"""
import numpy as np
import pytest
import torch

import text_segmentation_image_inpainting_amd as T
from tests.backends import BACKENDS, both_backends
from tests.test_region_crops import box_rect, random_page
from tests.test_region_paste import box_info, expected_paste, rgba

RECT = [box_rect(3, 5, 12, 30), box_rect(4, 6, 33, 12), box_rect(2, 2, 9, 9, (3, 3)), [-1, 0, 1, 7, 7, -5, -5, 1], box_rect(20, 20, 30, 44, (-2, 5))]
SIZE = (16, 48)


def want(page, info, slots, n=None, max_ss=4):
    slots = slots if slots.shape[-1] == 4 else rgba(slots)
    n = len(slots) if n is None else n
    return expected_paste(page, info, n, len(slots), slots, max_ss)[1]


@both_backends
def test_numpy_and_torch_in_and_out(backend):
    page, other = random_page(40, 50), random_page(40, 50, seed=11)
    slots = np.random.default_rng(5).integers(0, 256, size=(len(RECT), *SIZE, 4), dtype=np.uint8)
    with BACKENDS[backend]() as dev:
        rc = T.region_crops(page, np.array(RECT, np.int64), SIZE, device=dev)
        keep = (other.copy(), slots.copy(), rc.info.copy())
        a = T.paste_crops(other, slots, rc.info, device=dev)
        t_in = torch.from_numpy(other).to(dev)
        b = T.paste_crops(t_in, torch.from_numpy(slots).to(dev), torch.from_numpy(rc.info).to(dev), supersample=1, device=dev)
        assert torch.equal(t_in.cpu(), torch.from_numpy(keep[0])), "the page must not be modified"
        assert isinstance(b, torch.Tensor) and b.device == t_in.device and b.dtype == torch.uint8 and b.data_ptr() != t_in.data_ptr()
        b = b.cpu().numpy()
        c = T.paste_crops(torch.from_numpy(other), slots[..., :3], rc.info, n_rows=2, device=dev)
        d = T.paste_crops(other, slots, rc.info, n_rows=0, device=dev)
        e = T.paste_crops(other, slots[:0], rc.info[:0], device=dev)
        f = rc.paste(other, rc.crops, device=dev)
        g = rc.paste(other, slots, supersample=2, n_rows=3, device=dev)
    assert all(np.array_equal(x, y) for x, y in zip(keep, (other, slots, rc.info)))
    assert isinstance(a, np.ndarray) and a.dtype == np.uint8 and np.array_equal(a, want(other, rc.info, slots))
    assert np.array_equal(b, want(other, rc.info, slots, max_ss=1)) and not np.array_equal(a, b)
    assert isinstance(c, torch.Tensor) and c.device.type == "cpu", "a host tensor in, a host tensor out"
    assert np.array_equal(c.numpy(), want(other, rc.info, slots[..., :3], 2)), "three channels are opaque"
    for same in (d, e):
        assert isinstance(same, np.ndarray) and np.array_equal(same, other) and not np.shares_memory(same, other)
    assert np.array_equal(f, want(other, rc.info, rc.crops)) and np.array_equal(g, want(other, rc.info, slots, 3, 2))
    # the crops of a page pasted back opaque: the lettering's own pixels are back to within the resampling, everything far from them is not touched
    touched = (f != other).any(axis=-1)
    assert touched[3:13, 5:31].mean() > 0.9 and not touched[35:, :20].any()


@both_backends
def test_a_box_at_its_own_size_comes_back(backend):
    page, other = random_page(40, 60), random_page(40, 60, seed=11)
    with BACKENDS[backend]() as dev:
        rc = T.region_crops(page, np.array([box_rect(3, 5, 18, 52)], np.int64), SIZE, device=dev)
        out = rc.paste(other, rc.crops, device=dev)
    assert [int(v) for v in rc.info[0]] == box_info(3, 5, 16, 48)
    back = other.copy()
    back[3:19, 5:53] = page[3:19, 5:53]
    assert np.array_equal(out, back)


def test_arguments_are_checked():
    page, slots, info = np.zeros((8, 8, 3), np.uint8), np.zeros((2, 4, 4, 4), np.uint8), np.array([box_info(1, 1, 4, 4)] * 2, np.int32)
    for kw in (dict(supersample=0), dict(supersample=5), dict(supersample=1.5), dict(n_rows=3), dict(n_rows=-1), dict(n_rows=0.5)):
        with pytest.raises(ValueError):
            T.paste_crops(page, slots, info, **kw)
    for bad in (slots[..., :2], slots[0], slots.reshape(2, 4, 16), np.zeros((2, 4, 4097, 4), np.uint8), slots[:1]):
        with pytest.raises(ValueError, match="slots|info"):
            T.paste_crops(page, bad, info)
    for bad in (info[:, :9], info.reshape(-1), info[:1]):
        with pytest.raises(ValueError, match="info"):
            T.paste_crops(page, slots, bad)
    with pytest.raises(ValueError, match="int32"):
        T.paste_crops(page, slots, info.astype(np.int64))
    with pytest.raises(ValueError, match="uint8"):
        T.paste_crops(page, slots.astype(np.float32), info)
    with pytest.raises(ValueError, match="uint8"):
        T.paste_crops(page.astype(np.float32), slots, info)
    with pytest.raises(ValueError, match="uint8"):
        T.paste_crops(page[..., 0], slots, info)
    assert T.check_paste_args((2, 4, 4, 4), (2, 10), None, 4) == 2 and T.check_paste_args((2, 4, 4, 3), (2, 10), 1, 1) == 1
    assert T.check_paste_args((0, 4, 4, 4), (0, 10), None, 4) == 0
    with pytest.raises(ValueError, match="width"):
        T.check_paste_args((2, 4, 0, 4), (2, 10), None, 4)
