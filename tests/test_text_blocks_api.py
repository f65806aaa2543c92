"""``text_blocks`` (regions.py): the stand-alone form of K10 + K15, numpy or torch in and the same kind out, held to the restatement of
tests/test_text_blocks_kernels.py; bad arguments raise before any device work."""
import numpy as np
import pytest
import torch

import text_segmentation_image_inpainting_amd as T
from tests.backends import BACKENDS, both_backends
from tests.test_text_blocks_kernels import expected, k10_labels, pattern
from text_segmentation_image_inpainting_amd import regions


@both_backends
def test_text_blocks_round_trip(backend):
    text = pattern("noise0.02", 150, 217)
    mask = (text != 0).astype(np.uint8) * 255                        # what TextEraser returns
    keep = mask.copy()
    comps = {c: k10_labels(text, c) for c in (4, 8)}
    exp = expected(text, comps[8], 5, 4, None)
    exp4 = expected(text, comps[4], 1, 0, None)
    assert exp["n"][1] < exp["n"][0] < len(np.unique(comps[8])) - 1, "blocks are fewer than components, the filter drops some"
    with BACKENDS[backend]() as dev:
        r = T.text_blocks(mask, 5, min_area=4, device=dev)
        t_in = torch.from_numpy(mask).to(dev)
        rt = T.text_blocks(t_in, gap=5, connectivity=8, min_area=4, max_regions=7, device=dev)
        r4 = T.text_blocks(mask, 1, connectivity=4, device=dev)
        assert torch.equal(t_in.cpu(), torch.from_numpy(keep)), "the argument must not be modified"
        assert all(isinstance(v, torch.Tensor) and v.device == t_in.device for v in (rt.mask, rt.labels))
        assert rt.labels.dtype == torch.int32 and rt.mask.dtype == torch.uint8
        rt_labels, rt_mask = rt.labels.cpu().numpy(), rt.mask.cpu().numpy()
    assert np.array_equal(mask, keep)
    assert isinstance(r, T.TextBlocks) and isinstance(r.labels, np.ndarray) and r.labels.dtype == np.int32 and r.mask.dtype == np.uint8
    assert np.array_equal(r.labels, exp["labels"]) and np.array_equal(r.mask, exp["text"] * 255)
    assert np.array_equal(r.table, exp["table"]) and np.array_equal(r.members, exp["members"]) and r.table.dtype == r.members.dtype == np.int32
    assert (r.found, r.kept, r.components) == (exp["n"][0], exp["n"][1], len(np.unique(comps[8])) - 1)
    assert np.array_equal(rt_labels, exp["labels"]) and np.array_equal(rt_mask, exp["text"] * 255)
    assert np.array_equal(rt.table, exp["table"][:7]) and np.array_equal(rt.members, exp["members"][:7]) and rt.kept == exp["n"][1] > 7
    assert np.array_equal(r4.labels, exp4["labels"]) and np.array_equal(r4.members, exp4["members"])
    assert (r4.found, r4.kept, r4.components) == (exp4["n"][0], exp4["n"][1], len(np.unique(comps[4])) - 1)


def test_arguments_are_checked_before_any_device_work(monkeypatch):
    monkeypatch.setattr(regions, "call", lambda *a: pytest.fail("a kernel was called"))
    monkeypatch.setattr(regions, "_plane_on_device", lambda *a: pytest.fail("the plane went to the device"))
    mask = np.zeros((4, 4), np.uint8)
    for kw in (dict(gap=0), dict(gap=65), dict(gap=2.5), dict(gap=True), dict(gap=3, connectivity=6), dict(gap=3, min_area=-1),
               dict(gap=3, max_regions=0)):
        with pytest.raises(ValueError):
            T.text_blocks(mask, **kw)
    for gap in (0, 65, 1.5, True):
        with pytest.raises(ValueError, match="group"):
            T.TextEraser(lambda x: x, lambda x: x, device="cpu", group=gap)
    monkeypatch.undo()
    with pytest.raises(ValueError, match="uint8"):
        T.text_blocks(np.zeros((4, 4), np.float32), 3)
    assert T.TextEraser(lambda x: x, lambda x: x, device="cpu", group=12).regions
