"""``HarmonicFill`` and ``harmonic_fill`` (fill.py; ``tsii_harmonic_fill``, "K14: harmonic fill"): the ``filler`` convention of
``TextEraser`` and the stand-alone uint8 form, against the float64 restatement of ``tests/test_harmonic_kernels.py``.  Emulator (CPU
suite) and, with -m gpu, the chip."""
import numpy as np
import pytest
import torch

import text_segmentation_image_inpainting_amd as T
from tests.backends import BACKENDS, both_backends
from tests.test_harmonic_kernels import bound_of, case, harmonic_ref, holes
from tests.test_text_eraser import to_byte
from text_segmentation_image_inpainting_amd.masks import MaskParts

H, W = 150, 217


@both_backends
def test_mask_forms_and_memory_formats(backend):
    x, hole, ref = case("glyphs", 2, 65, 64, 8)
    with BACKENDS[backend]() as dev:
        fill = T.HarmonicFill()
        assert fill.sweeps == 8
        nhwc = torch.from_numpy(x).to(dev)
        plane = torch.from_numpy((~hole).astype(np.float32)).to(dev)
        cl = nhwc.permute(0, 3, 1, 2)                    # [N,3,H,W] in channels-last memory
        nchw = cl.contiguous()
        outs = [fill((cl, MaskParts.from_plane(plane, 3))), fill((nchw, plane)), fill((cl, plane.unsqueeze(1))),
                fill((nchw, plane.unsqueeze(1).expand(-1, 3, -1, -1))), fill((cl, plane.unsqueeze(1).repeat(1, 3, 1, 1))),
                fill((cl, (plane * 255).to(torch.uint8)))]
        for o in outs:
            assert tuple(o.shape) == (2, 3, 65, 64) and o.dtype == torch.float32 and o.device == nhwc.device
            assert o.permute(0, 2, 3, 1).is_contiguous(), "the NCHW-shaped view of the NHWC output"
        got = [o.permute(0, 2, 3, 1).cpu().numpy() for o in outs]
        per_channel = plane.unsqueeze(1).repeat(1, 3, 1, 1)
        per_channel[0, 1, 3, 3] = 1 - per_channel[0, 1, 3, 3]
        with pytest.raises(ValueError, match="per-channel"):
            fill((cl, per_channel))
        with pytest.raises(ValueError):
            fill((cl, plane[:, :10]))
        with pytest.raises(ValueError):
            fill((cl[:, :2], plane))
        if backend == "gpu":
            with pytest.raises(RuntimeError, match="no CPU path|GPU"):
                fill((cl.cpu(), plane.cpu()))
        zero = T.HarmonicFill(sweeps=0)((cl, plane)).permute(0, 2, 3, 1).cpu().numpy()
    for g in got[1:]:
        assert np.array_equal(g.view(np.uint32), got[0].view(np.uint32))
    assert float(np.abs(got[0] - ref).max()) <= bound_of(65, 64, 8, 1.0)
    assert float(np.abs(zero - case("glyphs", 2, 65, 64, 0)[2]).max()) <= bound_of(65, 64, 0, 1.0)
    for bad in (17, -1, 2.5, True):
        with pytest.raises(ValueError, match="sweeps"):
            T.HarmonicFill(sweeps=bad)
    assert not isinstance(T.HarmonicFill(), torch.nn.Module) and repr(T.HarmonicFill(3)) == "HarmonicFill(sweeps=3)"


@both_backends
def test_harmonic_fill_page(backend):
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = 0.2 + 0.5 * xx / W + 0.25 * yy / H
    exact = np.stack([ramp, 0.9 - 0.6 * ramp, 0.1 + 0.8 * ramp], axis=-1)
    page = to_byte(exact.astype(np.float32))
    hole = holes("glyphs", H, W, seed=3)
    hole[[0, -1]] = hole[:, [0, -1]] = False              # interior holes: the ramp is what belongs there
    assert 40 <= hole.sum() and hole.any(axis=1).sum() > 40
    mask = hole.astype(np.uint8) * 255
    keep_page, keep_mask = page.copy(), mask.copy()
    x = page.astype(np.float32) / np.float32(255.0)
    ref = harmonic_ref(x, ~hole, 8)
    bound = bound_of(H, W, 8, 1.0)
    with BACKENDS[backend]() as dev:
        clean = T.harmonic_fill(page, mask, device=dev)
        p_in, m_in = torch.from_numpy(page).to(dev), torch.from_numpy(mask // 255).to(dev)        # any non-zero byte removes
        clean_t = T.harmonic_fill(p_in, m_in, sweeps=8, device=dev)
        assert isinstance(clean_t, torch.Tensor) and clean_t.device == p_in.device and clean_t.dtype == torch.uint8
        assert torch.equal(p_in.cpu(), torch.from_numpy(keep_page)), "arguments are not modified"
        clean_t = clean_t.cpu().numpy()
        rough = T.harmonic_fill(page, mask, sweeps=0, device=dev)
    assert np.array_equal(page, keep_page) and np.array_equal(mask, keep_mask)
    assert isinstance(clean, np.ndarray) and clean.dtype == np.uint8 and clean.shape == (H, W, 3)
    assert np.array_equal(clean, clean_t)
    assert np.array_equal(clean[~hole], page[~hole]), "bytes outside the mask are identical"
    # inside: the restatement rounded the same way; a float within the bound of a .5 tie may round either way
    lo, hi = to_byte((ref - bound).astype(np.float32)), to_byte((ref + bound).astype(np.float32))
    inside = clean[hole].astype(int)
    assert bool((inside >= lo[hole]).all()) and bool((inside <= hi[hole]).all())
    assert int(np.abs(inside - to_byte(ref.astype(np.float32))[hole].astype(int)).max()) <= 1
    assert int(np.abs(inside - page_of(exact)[hole].astype(int)).max()) <= 2, "within 2 grey levels of the ramp"
    assert np.array_equal(rough[~hole], page[~hole]) and bool((rough != clean).any())


def page_of(exact):
    return to_byte(exact.astype(np.float32))


def test_arguments_are_checked():
    page, mask = np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.uint8)
    for bad in (-1, 17, 1.5):
        with pytest.raises(ValueError, match="sweeps"):
            T.harmonic_fill(page, mask, sweeps=bad)
    with pytest.raises(ValueError, match="uint8"):
        T.harmonic_fill(page.astype(np.float32), mask)
    with pytest.raises(ValueError, match="uint8"):
        T.harmonic_fill(page, mask.astype(np.float32))
    with pytest.raises(ValueError, match="mask must be"):
        T.harmonic_fill(page, np.zeros((4, 5), np.uint8))
    with pytest.raises(RuntimeError, match="no CPU path|GPU"):            # host tensors are refused: there is no CPU path
        T.harmonic_fill(page, mask, device="cpu")
