"""Text regions on the device: connected components of a text plane, their areas and boxes, and a minimum-area filter.

The counterpart of the reference demo's ``draw_bounding_box(origin_np, mask_np, 500)``: label the mask, drop the specks, say where the
text is.  One entry point, ``tsii_text_regions`` (``csrc/regions.hip``; semantics: ``include/tsii_hip.h``, "K10: text regions"); all
integer, so the result has the same bits on every run.  ``text_regions`` is the stand-alone form; ``TextEraser`` runs the same kernels
in place on its text plane between the mask and the tile selection (``pipeline.py``).
"""
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, ops
from ._lib import call, ptr


class TextRegions(NamedTuple):
    """``labels``: int32 ``[H, W]``, 0 = background or a dropped region, else ``1 + min(y * W + x)`` over the region's pixels.
    ``table``: numpy int32 ``[n, 6]``, one row ``(label, area, y0, x0, y1, x1)`` per kept region (``y1``, ``x1`` exclusive) in raster
    order of the regions' first pixels, ``n = min(kept, max_regions)``.  ``found`` / ``kept``: regions before / after the filter.
    ``truncated``: ``kept > max_regions``, the table holds the first ``max_regions`` rows only."""
    labels: object
    table: np.ndarray
    found: int
    kept: int
    truncated: bool


def check_region_args(connectivity, min_area, max_regions):
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity {connectivity} must be 4 or 8")
    if int(min_area) != min_area or min_area < 0:
        raise ValueError(f"min_area {min_area} must be an integer >= 0")
    if int(max_regions) != max_regions or max_regions < 1:
        raise ValueError(f"max_regions {max_regions} must be an integer >= 1")


def _text_regions(text, connectivity, min_area, max_regions, grid=None):
    """``tsii_text_regions`` in place on the device plane ``text`` -> (labels, packed): ``packed`` is ONE int32 device tensor
    ``[core counts (grid.count, with a grid) | found, kept | table rows]``, so that a caller reads everything back with one copy."""
    h, w = int(text.shape[0]), int(text.shape[1])
    _lib.check_device(text.new_empty(0, dtype=torch.float32))
    assert text.dtype == torch.uint8 and text.is_contiguous()
    nbytes = int(_lib.lib().tsii_text_regions_ws_bytes(h, w, int(max_regions)))
    if nbytes == 0:
        raise ValueError(f"text plane of {h} x {w} pixels is out of range")
    nt = 0 if grid is None else grid.count
    labels = torch.empty((h, w), dtype=torch.int32, device=text.device)
    packed = torch.zeros((nt + 2 + 6 * int(max_regions),), dtype=torch.int32, device=text.device)
    ws = ops._ws(nbytes, text)
    tile, halo = (0, 0) if grid is None else (grid.tile, grid.halo)
    call("tsii_text_regions", ptr(text), h, w, int(connectivity), int(min_area), int(max_regions), tile, halo,
         ptr(packed[:nt]) if nt else None, ptr(labels), ptr(packed[nt + 2:]), ptr(packed[nt:nt + 2]), ptr(ws), _lib.stream())
    return labels, packed


def unpack_regions(packed_h, nt, max_regions):
    """host copy of ``packed`` -> (core counts, table, found, kept, truncated)"""
    found, kept = int(packed_h[nt]), int(packed_h[nt + 1])
    n = min(kept, int(max_regions))
    table = packed_h[nt + 2:nt + 2 + 6 * n].reshape(n, 6).copy()
    return packed_h[:nt], table, found, kept, kept > n


def text_regions(text, connectivity=8, min_area=0, max_regions=4096, device=None) -> TextRegions:
    """Connected regions of a text plane.  ``text``: ``[H, W]`` uint8, numpy or torch, host or device; non-zero = text (the 255
    masks ``TextEraser`` returns work directly).  The argument is not modified.  Regions of fewer than ``min_area`` pixels are
    dropped.  ``labels`` comes back the same kind and on the same device as ``text``; one synchronisation (the read-back of the
    counts and the table).  A host plane is computed on ``device`` (default ``cuda:0``)."""
    check_region_args(connectivity, min_area, max_regions)
    t = torch.from_numpy(np.ascontiguousarray(text)) if isinstance(text, np.ndarray) else text
    if t.dim() != 2 or t.dtype != torch.uint8 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"text must be [H, W] uint8, got {tuple(t.shape)} {t.dtype}")
    dev = torch.device(device) if device is not None else (t.device if t.is_cuda else torch.device("cuda:0"))
    plane = t.to(dev, copy=True).contiguous()
    labels, packed = _text_regions(plane, connectivity, min_area, max_regions)
    _, table, found, kept, truncated = unpack_regions(packed.cpu().numpy(), 0, max_regions)
    if isinstance(text, np.ndarray):
        labels = labels.cpu().numpy()
    elif labels.device != text.device:
        labels = labels.to(text.device)
    return TextRegions(labels, table, found, kept, truncated)

